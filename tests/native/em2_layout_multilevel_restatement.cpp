// em2_layout_multilevel_restatement.cpp -- the multilevel spring-electrical layout on one thread, in plain
// loops: what em2_graph_layout_multilevel, em2_graph_layout_coarsen and em2_graph_layout_forces_weighted of
// csrc/em2_layout.hip must equal bit for bit.  The matching is stated as what it is, the greedy matching over the edges sorted
// by their key, never as the rounds the device runs; the number of rounds the device needs is derived from that order (an edge
// is matched one round after the last vertex that a better edge at one of its ends leads to).  Every floating-point operation
// and the order of every sum is written out as include/em2_lsh.h states them; compile with -ffp-contract=off so that nothing
// fuses except the fmaf calls.  Includes nothing of the library.  Test infrastructure only.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <tuple>
#include <vector>

namespace {

constexpr float kC = 0.2f;                 // C * K^2 with K = 1
constexpr float kFloor = 1e-30f;           // delta
constexpr double kT = 0.9;
constexpr uint32_t kChunk = 256;
constexpr uint32_t kSliceCount = 16;
constexpr uint32_t kLeafTarget = 8;
constexpr uint32_t kMaxDepth = 10;
constexpr uint32_t kDepthAuto = 0xffffffffu;
constexpr uint32_t kDepthExact = 0xfffffffeu;
constexpr uint32_t kCoarsest = 32;
constexpr uint32_t kMaxLevels = 32;
constexpr uint32_t kExactLimit = 4096;
constexpr uint32_t kNone = 0xffffffffu;

uint64_t mix(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

uint64_t levelHash(uint32_t seed, uint32_t level, uint64_t what) { return mix(mix(uint64_t(seed) << 32 | level) ^ what); }

// u in [-0.5, 0.5)^2 from the hash z, 24 bits per coordinate.
void unitSquare(uint64_t z, float* ux, float* uy)
{
    *ux = float(uint32_t(z >> 40)) * 0x1p-24f - 0.5f;
    *uy = float(uint32_t(z >> 16) & 0xffffffu) * 0x1p-24f - 0.5f;
}

uint32_t automaticDepth(uint32_t n)
{
    for (uint32_t depth = 0; depth < kMaxDepth; depth++) {
        if ((uint64_t(kLeafTarget) << (2 * depth)) >= n) return depth;
    }
    return kMaxDepth;
}

// A graph as the force reads it: per vertex a mass and the neighbours ascending, each with a weight.  Level 0 of a run has
// mass 1, weight 1 and a repeated input edge as two entries; a coarse level has merged edges, so distinct neighbours.
struct Graph {
    uint32_t n = 0;
    std::vector<float> mass;                // float(the integer mass)
    std::vector<uint32_t> integerMass;
    std::vector<uint64_t> offsets;
    std::vector<uint32_t> neighbours;
    std::vector<float> weights;
    // (stable in the order of the edges where two entries of a vertex name the same neighbour)
    Graph(uint32_t n_, const uint32_t* mass_, const uint32_t* e0, const uint32_t* e1, const uint32_t* w, uint64_t edgeCount)
        : n(n_), mass(n_, 1.f), integerMass(n_, 1u), offsets(size_t(n_) + 1, 0)
    {
        if (mass_) {
            integerMass.assign(mass_, mass_ + n);
            for (uint32_t v = 0; v < n; v++) mass[v] = float(mass_[v]);
        }
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> lists(n);
        for (uint64_t e = 0; e < edgeCount; e++) {
            lists[e0[e]].push_back({e1[e], w ? w[e] : 1u});
            lists[e1[e]].push_back({e0[e], w ? w[e] : 1u});
        }
        for (uint32_t v = 0; v < n; v++) {
            std::stable_sort(lists[v].begin(), lists[v].end(), [](const auto& a, const auto& b) { return a.first < b.first; });
            offsets[v + 1] = offsets[v] + lists[v].size();
            for (const auto& entry : lists[v]) {
                neighbours.push_back(entry.first);
                weights.push_back(float(entry.second));
            }
        }
    }
};

// ---- coarsening: integers only ----

struct Edge {
    uint32_t a, b, w;                       // a < b
};

// The merged edges of arbitrary input edges: self-loops dropped, (a, b) and (b, a) the same edge, weights added; ascending.
std::vector<Edge> mergeEdges(const uint32_t* e0, const uint32_t* e1, const uint32_t* w, uint64_t edgeCount)
{
    std::vector<Edge> all;
    for (uint64_t e = 0; e < edgeCount; e++) {
        if (e0[e] == e1[e]) continue;
        all.push_back({std::min(e0[e], e1[e]), std::max(e0[e], e1[e]), w ? w[e] : 1u});
    }
    std::sort(all.begin(), all.end(), [](const Edge& x, const Edge& y) { return std::tie(x.a, x.b) < std::tie(y.a, y.b); });
    std::vector<Edge> merged;
    for (const Edge& e : all) {
        if (!merged.empty() && merged.back().a == e.a && merged.back().b == e.b) merged.back().w += e.w;
        else merged.push_back(e);
    }
    return merged;
}

typedef std::tuple<uint32_t, uint64_t, uint32_t, uint32_t> Key;

Key keyOf(const Edge& e, uint32_t seed, uint32_t level) { return Key(e.w, levelHash(seed, level, uint64_t(e.a) << 32 | e.b), e.a, e.b); }

// The greedy matching over the edges in descending key order.  *rounds: how many rounds of locally dominant edges find it.
std::vector<uint32_t> greedyMatching(uint32_t n, const std::vector<Edge>& edges, uint32_t seed, uint32_t level, uint32_t* rounds)
{
    std::vector<std::pair<Key, uint32_t>> order;
    std::vector<std::vector<std::pair<Key, uint32_t>>> incident(n);      // per vertex: (key, other end)
    for (uint32_t e = 0; e < edges.size(); e++) {
        const Key key = keyOf(edges[e], seed, level);
        order.push_back({key, e});
        incident[edges[e].a].push_back({key, edges[e].b});
        incident[edges[e].b].push_back({key, edges[e].a});
    }
    std::sort(order.begin(), order.end(), [](const auto& x, const auto& y) { return x.first > y.first; });
    std::vector<uint32_t> mate(n, kNone), roundOf(n, 0);
    *rounds = 0;
    for (const auto& entry : order) {
        const Edge& e = edges[entry.second];
        if (mate[e.a] != kNone || mate[e.b] != kNone) continue;
        // every better edge at a or b was passed over because its other end was matched already: e waits for the last of them
        uint32_t round = 1;
        for (uint32_t end : {e.a, e.b}) {
            for (const auto& other : incident[end]) {
                if (other.first > entry.first) round = std::max(round, roundOf[other.second] + 1);
            }
        }
        mate[e.a] = e.b;
        mate[e.b] = e.a;
        roundOf[e.a] = roundOf[e.b] = round;
        *rounds = std::max(*rounds, round);
    }
    return mate;
}

struct Level {
    uint32_t n = 0;
    std::vector<uint32_t> mass;
    std::vector<Edge> edges;
    // towards the next level (empty at the coarsest)
    std::vector<uint32_t> mate, coarseOf;
    uint32_t rounds = 0;                    // of the matching that made this level from the one below it
};

// One coarsening step of `fine`: fills fine.mate and fine.coarseOf, returns the next level.
Level coarsen(Level& fine, uint32_t seed, uint32_t levelIndex)
{
    Level coarse;
    fine.mate = greedyMatching(fine.n, fine.edges, seed, levelIndex, &coarse.rounds);
    fine.coarseOf.assign(fine.n, 0);
    for (uint32_t v = 0; v < fine.n; v++) {
        if (fine.mate[v] == kNone || v < fine.mate[v]) {
            fine.coarseOf[v] = coarse.n++;
            coarse.mass.push_back(fine.mass[v] + (fine.mate[v] == kNone ? 0u : fine.mass[fine.mate[v]]));
        } else {
            fine.coarseOf[v] = fine.coarseOf[fine.mate[v]];
        }
    }
    std::vector<uint32_t> a, b, w;
    for (const Edge& e : fine.edges) {
        a.push_back(fine.coarseOf[e.a]);
        b.push_back(fine.coarseOf[e.b]);
        w.push_back(e.w);
    }
    coarse.edges = mergeEdges(a.data(), b.data(), w.data(), a.size());
    return coarse;
}

std::vector<Level> hierarchy(uint32_t n, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, uint32_t seed)
{
    std::vector<Level> levels(1);
    levels[0].n = n;
    levels[0].mass.assign(n, 1u);
    levels[0].edges = mergeEdges(e0, e1, nullptr, edgeCount);
    while (levels.back().n > kCoarsest && levels.size() < kMaxLevels) {
        Level next = coarsen(levels.back(), seed, uint32_t(levels.size() - 1));
        if (4ull * next.n > 3ull * levels.back().n) {
            levels.back().mate.clear();
            levels.back().coarseOf.clear();
            break;
        }
        levels.push_back(std::move(next));
    }
    return levels;
}

// ---- the force ----

double tree256(double* v)
{
    for (uint32_t stride = kChunk / 2; stride >= 1; stride /= 2) {
        for (uint32_t t = 0; t < stride; t++) v[t] += v[t + stride];
    }
    return v[0];
}

uint32_t levelBegin(uint32_t level) { return ((1u << (2 * level)) - 1) / 3; }

uint32_t quantise(float v, float lo, float side)
{
    if (side == 0.f) return 0;
    const float u = fminf(fmaxf((v - lo) / side, 0.f), 1.f);
    return uint32_t(u * 2147483648.f);
}

// The pyramid of one evaluation with masses: a cell's count is its mass sum, its moments the sums of m * q.
struct Pyramid {
    uint32_t depth = 0;
    float xmin = 0.f, ymin = 0.f, side = 0.f;
    std::vector<uint32_t> qx, qy;
    std::vector<uint32_t> count;
    std::vector<uint64_t> sumX, sumY;
    std::vector<float> mx, my;
    std::vector<uint32_t> leafBegin, leafVertices;

    uint32_t cellOf(uint32_t q, uint32_t level) const { return std::min((1u << level) - 1, q >> (31 - level)); }

    Pyramid(const Graph& g, uint32_t depth_, const float* x, const float* y) : depth(depth_), qx(g.n), qy(g.n)
    {
        const uint32_t n = g.n;
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
        std::vector<uint32_t> leafOf(n), vertices(leaves, 0);
        for (uint32_t i = 0; i < n; i++) {
            qx[i] = quantise(x[i], xmin, side);
            qy[i] = quantise(y[i], ymin, side);
            leafOf[i] = cellOf(qy[i], depth) << depth | cellOf(qx[i], depth);
            const uint32_t c = levelBegin(depth) + leafOf[i];
            const uint32_t m = g.integerMass[i];
            count[c] += m;
            sumX[c] += uint64_t(m) * qx[i];
            sumY[c] += uint64_t(m) * qy[i];
            vertices[leafOf[i]]++;
        }
        leafBegin.assign(size_t(leaves) + 1, 0);
        for (uint32_t c = 0; c < leaves; c++) leafBegin[c + 1] = leafBegin[c] + vertices[c];
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

inline __attribute__((always_inline)) void repel(float xi, float yi, float xj, float yj, float mj, float& fx, float& fy)
{
    const float dx = xi - xj, dy = yi - yj;
    const float d2 = fmaf(dx, dx, dy * dy);
    const float w = (kC * mj) / fmaxf(d2, kFloor);
    fx = fmaf(dx, w, fx);
    fy = fmaf(dy, w, fy);
}

// f for the positions (x, y); returns the energy.  depth: kDepthExact or the depth of the pyramid.  terms (may be null): the
// addends of each vertex's repulsion sums.
inline __attribute__((always_inline)) double forcesBody(const Graph& g, float gravity, uint32_t depth, const float* x, const float* y, float* fx,
                                                        float* fy, uint32_t* terms)
{
    const uint32_t n = g.n;
    const bool exact = depth == kDepthExact;
    const Pyramid pyramid(g, exact ? 0u : depth, x, y);
    const uint32_t sliceLength = (n + kSliceCount - 1) / kSliceCount;
    std::vector<double> chunkEnergy;
    double leaves[kChunk];
    for (uint32_t i = 0; i < n; i++) {
        const float xi = x[i], yi = y[i];
        uint32_t termCount = 0;
        float rx = 0.f, ry = 0.f;
        if (exact) {
            for (uint32_t s = 0; s < kSliceCount; s++) {
                const uint64_t begin = std::min<uint64_t>(uint64_t(s) * sliceLength, n);
                const uint64_t end = std::min<uint64_t>(begin + sliceLength, n);
                float px = 0.f, py = 0.f;
                for (uint64_t j = begin; j < end; j++) repel(xi, yi, x[j], y[j], g.mass[j], px, py);
                if (s == 0) {
                    rx = px;
                    ry = py;
                } else {
                    rx += px;
                    ry += py;
                }
            }
            termCount = n;
        } else {
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
                        repel(xi, yi, pyramid.mx[c], pyramid.my[c], float(pyramid.count[c]), farX, farY);
                        termCount++;
                    }
                }
            }
            float nearX = 0.f, nearY = 0.f;
            const int64_t width = int64_t(1) << depth;
            const int64_t ax = pyramid.cellOf(pyramid.qx[i], depth), ay = pyramid.cellOf(pyramid.qy[i], depth);
            for (int64_t by = ay - 1; by <= ay + 1; by++) {
                for (int64_t bx = ax - 1; bx <= ax + 1; bx++) {
                    if (bx < 0 || by < 0 || bx >= width || by >= width) continue;
                    const uint32_t leaf = uint32_t(by * width + bx);
                    for (uint32_t k = pyramid.leafBegin[leaf]; k < pyramid.leafBegin[leaf + 1]; k++) {
                        const uint32_t j = pyramid.leafVertices[k];
                        repel(xi, yi, x[j], y[j], g.mass[j], nearX, nearY);
                        termCount++;
                    }
                }
            }
            rx = farX + nearX;
            ry = farY + nearY;
        }
        if (terms) terms[i] = termCount;
        float ax = 0.f, ay = 0.f;
        for (uint64_t k = g.offsets[i]; k < g.offsets[i + 1]; k++) {
            const uint32_t j = g.neighbours[k];
            const float dx = xi - x[j], dy = yi - y[j];
            const float d = sqrtf(fmaf(dx, dx, dy * dy));
            ax = fmaf(dx, d * g.weights[k], ax);
            ay = fmaf(dy, d * g.weights[k], ay);
        }
        float fxi = rx - ax / g.mass[i], fyi = ry - ay / g.mass[i];
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

// What a level of n vertices evaluates its repulsion with, from the entry's depth argument.
uint32_t depthOfLevel(uint32_t depth, uint32_t level, uint32_t n)
{
    if (depth == kDepthExact) return kDepthExact;
    if (depth != kDepthAuto) return std::min(depth, kMaxDepth);
    return level > 0 && n <= kExactLimit ? kDepthExact : automaticDepth(n);
}

struct Run {
    uint32_t iterations = 0;
    double step = 0., energy = 0.;
};

// Hu's adaptive iteration on one level, from the positions in x / y.
Run iterate(const Graph& g, uint32_t depth, uint32_t maxIterationCount, double tolerance, double gravity, double initialStep, float* x,
            float* y)
{
    const uint32_t n = g.n;
    Run run;
    run.step = initialStep;
    run.energy = std::numeric_limits<double>::infinity();
    uint32_t progress = 0;
    std::vector<float> fx(n), fy(n), nx(n), ny(n);
    while (run.iterations < maxIterationCount && !(run.step < tolerance)) {
        const double energy0 = run.energy;
        run.energy = forces(g, float(gravity), depth, x, y, fx.data(), fy.data(), nullptr);
        const float stepF = float(run.step);
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
        if (run.energy < energy0) {
            if (++progress >= 5) {
                progress = 0;
                run.step /= kT;
            }
        } else {
            progress = 0;
            run.step *= kT;
        }
        run.iterations++;
    }
    return run;
}

}  // namespace

extern "C" {

// One coarsening step of the graph (n vertices; arbitrary edges with optional weights, NULL = 1; optional masses, NULL = 1).
// mate / coarseOf [n]; coarseMass [n] and coarseEdge0 / coarseEdge1 / coarseWeight [edgeCount] are filled from the front.
// counts: [0] the coarse vertices, [1] the rounds, [2] the coarse edges.
void em2rm_coarsen(uint32_t n, const uint32_t* mass, const uint32_t* e0, const uint32_t* e1, const uint32_t* w, uint64_t edgeCount,
                   uint32_t seed, uint32_t level, uint32_t* mate, uint32_t* coarseOf, uint32_t* coarseMass, uint32_t* coarseEdge0,
                   uint32_t* coarseEdge1, uint32_t* coarseWeight, uint64_t* counts)
{
    Level fine;
    fine.n = n;
    fine.mass.assign(n, 1u);
    if (mass) fine.mass.assign(mass, mass + n);
    fine.edges = mergeEdges(e0, e1, w, edgeCount);
    const Level coarse = coarsen(fine, seed, level);
    std::copy(fine.mate.begin(), fine.mate.end(), mate);
    std::copy(fine.coarseOf.begin(), fine.coarseOf.end(), coarseOf);
    std::copy(coarse.mass.begin(), coarse.mass.end(), coarseMass);
    for (size_t e = 0; e < coarse.edges.size(); e++) {
        coarseEdge0[e] = coarse.edges[e].a;
        coarseEdge1[e] = coarse.edges[e].b;
        coarseWeight[e] = coarse.edges[e].w;
    }
    counts[0] = coarse.n;
    counts[1] = coarse.rounds;
    counts[2] = coarse.edges.size();
}

// One evaluation with masses and edge weights (NULL = 1); depth: 0xfffffffe exact, 0xffffffff the automatic depth, or a depth.
void em2rm_forces_weighted(uint32_t n, const uint32_t* mass, const uint32_t* e0, const uint32_t* e1, const uint32_t* w, uint64_t edgeCount,
                           double gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy, double* energy, uint32_t* terms)
{
    const Graph g(n, mass, e0, e1, w, edgeCount);
    const uint32_t d = depth == kDepthExact ? kDepthExact : depth == kDepthAuto ? automaticDepth(n) : std::min(depth, kMaxDepth);
    const double e = n ? forces(g, float(gravity), d, x, y, fx, fy, terms) : 0.;
    if (energy) *energy = e;
}

// The run.  result: [0] the iterations of all levels, [1] the final step, [2] the final energy of level 0.  levelCount and, per
// level [32]: the vertices, the merged edges, the rounds of the matching that made the level, the iterations.
void em2rm_layout(uint32_t n, const uint32_t* e0, const uint32_t* e1, uint64_t edgeCount, uint32_t seed, uint32_t maxIterationCount,
                  double tolerance, double gravity, double initialStep, uint32_t depth, float* x, float* y, double* result, uint32_t* levelCount,
                  uint32_t* levelVertices, uint64_t* levelEdges, uint32_t* levelRounds, uint32_t* levelIterations)
{
    result[0] = 0.;
    result[1] = initialStep;
    result[2] = std::numeric_limits<double>::infinity();
    *levelCount = 0;
    if (!n) return;
    const std::vector<Level> levels = hierarchy(n, e0, e1, edgeCount, seed);
    *levelCount = uint32_t(levels.size());
    const uint32_t last = uint32_t(levels.size() - 1);
    std::vector<float> px(levels[last].n), py(levels[last].n);
    const float side = sqrtf(float(n));
    for (uint32_t i = 0; i < levels[last].n; i++) {
        float ux, uy;
        unitSquare(mix(uint64_t(seed) << 32 | i), &ux, &uy);
        px[i] = ux * side;
        py[i] = uy * side;
    }
    uint32_t total = 0;
    for (uint32_t l = last;; l--) {
        const Level& level = levels[l];
        if (l < last) {
            // a group's representative takes the group's position, its other member a hashed offset from it
            std::vector<float> fineX(level.n), fineY(level.n);
            for (uint32_t v = 0; v < level.n; v++) {
                fineX[v] = px[level.coarseOf[v]];
                fineY[v] = py[level.coarseOf[v]];
                if (level.mate[v] != kNone && level.mate[v] < v) {
                    float ux, uy;
                    unitSquare(levelHash(seed, l, v), &ux, &uy);
                    fineX[v] += ux;
                    fineY[v] += uy;
                }
            }
            px.swap(fineX);
            py.swap(fineY);
        }
        std::vector<uint32_t> a, b, w;
        for (const Edge& e : level.edges) {
            a.push_back(e.a);
            b.push_back(e.b);
            w.push_back(e.w);
        }
        // level 0 is the input as it is: unit masses, a repeated edge twice, self-loops (which add exact zeros)
        const Graph g = l ? Graph(level.n, level.mass.data(), a.data(), b.data(), w.data(), a.size()) : Graph(n, nullptr, e0, e1, nullptr, edgeCount);
        const Run run = iterate(g, depthOfLevel(depth, l, level.n), maxIterationCount, tolerance, gravity, initialStep, px.data(), py.data());
        levelVertices[l] = level.n;
        levelEdges[l] = level.edges.size();
        levelRounds[l] = level.rounds;
        levelIterations[l] = run.iterations;
        total += run.iterations;
        if (l == 0) {
            result[1] = run.step;
            result[2] = run.energy;
            break;
        }
    }
    result[0] = double(total);
    memcpy(x, px.data(), size_t(n) * sizeof(float));
    memcpy(y, py.data(), size_t(n) * sizeof(float));
}

}  // extern "C"
