// em2_gene_pairs_restatement.cpp -- ExpressionMatrix::findSimilarGenePairs0 restated for one thread, line by line:
//   src/ExpressionMatrixSubset.cpp:47-58     computeSums
//   src/ExpressionMatrixSubset.cpp:142-174   getDenseRepresentation
//   src/ExpressionMatrixFindSimilarGenePairs.cpp:117-188   standardisation, the pair loop, keepBest and sort
//   src/heap.hpp:116-126                     keepBest
// with the real std::inner_product, std::nth_element and std::sort.  Test infrastructure: what the device is compared with.
// Build: g++ -std=c++17 -O2 -msse4.2 -ffp-contract=off -fPIC -shared (tests/gene_pairs_binding.py).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <utility>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

typedef std::pair<uint32_t, float> Pair;

struct OrderPairsBySecondGreater {                                   // src/orderPairs.hpp:56-62
    bool operator()(const Pair& x, const Pair& y) const { return x.second > y.second; }
};

template <class T, class Compare> void keepBest(std::vector<T>& v, size_t k, const Compare& comparator)     // src/heap.hpp:116-126
{
    if (v.size() > k) {
        std::nth_element(v.begin(), v.begin() + k, v.end(), comparator);
        v.resize(k);
    }
}

}  // namespace

extern "C" {

// method: 0 none, 1 L1, 2 L2.  outGene / outSimilarity [geneCount][k] (unused slots zero), usedCount [geneCount];
// allSimilarities: NULL or [geneCount][geneCount], r of every pair, the diagonal 0.  Returns 0, or 1 for bad arguments.
int em2r_find_similar_gene_pairs0(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneCount, int method,
                                  uint32_t k, double similarityThreshold, uint32_t* outGene, float* outSimilarity,
                                  uint32_t* usedCount, float* allSimilarities)
{
    if (method < 0 || method > 2 || cellCount == 0 || geneCount == 0) return 1;

    // computeSums
    std::vector<double> sum1(cellCount, 0.), sum2(cellCount, 0.);
    for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) {
            if (data[p].gene >= geneCount) return 1;
            const float& count = data[p].count;
            sum1[cellId] += count;
            sum2[cellId] += count * count;
        }
    }

    // getDenseRepresentation
    std::vector<std::vector<float> > v(geneCount, std::vector<float>(cellCount, 0.));
    for (uint32_t cellId = 0; cellId != cellCount; ++cellId) {
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) v[data[p].gene][cellId] = data[p].count;
    }
    if (method != 0) {
        for (uint32_t cellId = 0; cellId != cellCount; cellId++) {
            const double scaling = (method == 1) ? sum1[cellId] : std::sqrt(sum2[cellId]);
            if (scaling != 0.) {
                const float factor = float(1. / scaling);
                for (uint32_t geneId = 0; geneId != geneCount; geneId++) v[geneId][cellId] *= factor;
            }
        }
    }

    // zero mean and unit variance
    for (uint32_t geneId = 0; geneId != geneCount; geneId++) {
        std::vector<float>& x = v[geneId];
        double sum = 0.;
        for (float count : x) sum += count;
        const float average = float(sum / cellCount);
        for (float& count : x) count -= average;
        double sumOfSquares = 0.;
        for (float count : x) sumOfSquares += count * count;
        const float factor = float(1. / std::sqrt(sumOfSquares));
        for (float& count : x) count *= factor;
    }

    // the loop over gene pairs
    std::vector<std::vector<Pair> > similarGenes(geneCount);
    if (allSimilarities) std::fill(allSimilarities, allSimilarities + size_t(geneCount) * geneCount, 0.f);
    for (uint32_t geneId0 = 1; geneId0 != geneCount; geneId0++) {
        std::vector<float>& x0 = v[geneId0];
        for (uint32_t geneId1 = 0; geneId1 != geneId0; geneId1++) {
            std::vector<float>& x1 = v[geneId1];
            const float r = std::inner_product(x0.begin(), x0.end(), x1.begin(), 0.f);
            if (r > similarityThreshold) {
                similarGenes[geneId0].push_back(std::make_pair(geneId1, r));
                similarGenes[geneId1].push_back(std::make_pair(geneId0, r));
            }
            if (allSimilarities) {
                allSimilarities[size_t(geneId0) * geneCount + geneId1] = r;
                allSimilarities[size_t(geneId1) * geneCount + geneId0] = r;
            }
        }
    }

    // keep the k best of every gene and sort them
    for (uint32_t geneId = 0; geneId != geneCount; geneId++) {
        std::vector<Pair>& list = similarGenes[geneId];
        keepBest(list, size_t(k), OrderPairsBySecondGreater());
        std::sort(list.begin(), list.end(), OrderPairsBySecondGreater());
        usedCount[geneId] = uint32_t(list.size());
        for (size_t i = 0; i < size_t(k); i++) {
            outGene[size_t(geneId) * k + i] = i < list.size() ? list[i].first : 0u;
            outSimilarity[size_t(geneId) * k + i] = i < list.size() ? list[i].second : 0.f;
        }
    }
    return 0;
}

// The same r for the genes [geneBegin, geneEnd) against all genes below each (a band of the triangle: timing and parity of
// large inputs): out[(g0 - geneBegin) * geneCount + g1] for g1 < g0.  *seconds receives the time of the inner products alone.
int em2r_gene_pair_band(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneCount, int method,
                        uint32_t geneBegin, uint32_t geneEnd, float* out, double* seconds);

// keepBest and sort (src/ExpressionMatrixFindSimilarGenePairs.cpp:183-187) for one gene whose r to the partners
// 0 .. partnerCount-1 is given and which has no other partner (the LAST gene of a problem, from em2r_gene_pair_band): its
// candidates in ascending partner id, the real std::nth_element and std::sort.  outGene / outSimilarity [k], unused slots zero.
int em2r_keep_best_and_sort(const float* r, uint32_t partnerCount, uint32_t k, double similarityThreshold, uint32_t* outGene,
                            float* outSimilarity, uint32_t* usedCount);

}  // extern "C"

int em2r_keep_best_and_sort(const float* r, uint32_t partnerCount, uint32_t k, double similarityThreshold, uint32_t* outGene,
                            float* outSimilarity, uint32_t* usedCount)
{
    std::vector<Pair> list;
    for (uint32_t geneId1 = 0; geneId1 != partnerCount; geneId1++) {
        if (r[geneId1] > similarityThreshold) list.push_back(std::make_pair(geneId1, r[geneId1]));
    }
    keepBest(list, size_t(k), OrderPairsBySecondGreater());
    std::sort(list.begin(), list.end(), OrderPairsBySecondGreater());
    *usedCount = uint32_t(list.size());
    for (size_t i = 0; i < size_t(k); i++) {
        outGene[i] = i < list.size() ? list[i].first : 0u;
        outSimilarity[i] = i < list.size() ? list[i].second : 0.f;
    }
    return 0;
}

#include <chrono>

int em2r_gene_pair_band(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneCount, int method,
                        uint32_t geneBegin, uint32_t geneEnd, float* out, double* seconds)
{
    if (method < 0 || method > 2 || cellCount == 0 || geneCount == 0 || geneBegin > geneEnd || geneEnd > geneCount) return 1;
    std::vector<double> sum1(cellCount, 0.), sum2(cellCount, 0.);
    for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) {
            if (data[p].gene >= geneCount) return 1;
            const float& count = data[p].count;
            sum1[cellId] += count;
            sum2[cellId] += count * count;
        }
    }
    // only the genes below geneEnd take part
    std::vector<std::vector<float> > v(geneEnd, std::vector<float>(cellCount, 0.));
    for (uint32_t cellId = 0; cellId != cellCount; ++cellId) {
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) {
            if (data[p].gene < geneEnd) v[data[p].gene][cellId] = data[p].count;
        }
    }
    if (method != 0) {
        for (uint32_t cellId = 0; cellId != cellCount; cellId++) {
            const double scaling = (method == 1) ? sum1[cellId] : std::sqrt(sum2[cellId]);
            if (scaling != 0.) {
                const float factor = float(1. / scaling);
                for (uint32_t geneId = 0; geneId != geneEnd; geneId++) v[geneId][cellId] *= factor;
            }
        }
    }
    for (uint32_t geneId = 0; geneId != geneEnd; geneId++) {
        std::vector<float>& x = v[geneId];
        double sum = 0.;
        for (float count : x) sum += count;
        const float average = float(sum / cellCount);
        for (float& count : x) count -= average;
        double sumOfSquares = 0.;
        for (float count : x) sumOfSquares += count * count;
        const float factor = float(1. / std::sqrt(sumOfSquares));
        for (float& count : x) count *= factor;
    }
    const auto begin = std::chrono::steady_clock::now();
    for (uint32_t geneId0 = geneBegin; geneId0 != geneEnd; geneId0++) {
        std::vector<float>& x0 = v[geneId0];
        for (uint32_t geneId1 = 0; geneId1 != geneId0; geneId1++) {
            std::vector<float>& x1 = v[geneId1];
            out[size_t(geneId0 - geneBegin) * geneCount + geneId1] = std::inner_product(x0.begin(), x0.end(), x1.begin(), 0.f);
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    return 0;
}
