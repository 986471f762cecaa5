// em2_dense_restatement.cpp -- the checker of the dense read-out and of the cell set operations: a restatement, line by line,
// of what the reference does, written from reading it; no text of the reference is in here.
//
//   em2r_dense_expression   ExpressionMatrix::getDenseExpressionMatrix after its lookups (src/PythonModule.cpp:112-138) on an
//                           ExpressionMatrixSubset given as a CSR in local ids, with the subset's sums computed as
//                           ExpressionMatrixSubset::computeSums does (src/ExpressionMatrixSubset.cpp:47-58).
//   em2r_deduplicate        deduplicate (src/deduplicate.hpp:9-13): what CellSets::addCellSet stores (src/CellSets.cpp:65-83).
//   em2r_set_operation      one step of createCellSetIntersectionOrUnion (src/ExpressionMatrix.cpp:1676-1688) or
//                           createCellSetDifference (:1727-1731).
//   em2r_downsample         downsampleCellSet (:1757-1772): boost::mt19937 has std::mt19937's parameters, and
//                           boost::uniform_01<> over a 32-bit integer engine returns one draw times 2^-32.
//
// Built by tests/dense_binding.py with g++ -O2 -ffp-contract=off for plain x86-64: no FMA can form.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <iterator>
#include <random>
#include <utility>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

struct Sum {
    double sum1 = 0.;
    double sum2 = 0.;
};

}  // namespace

extern "C" {

// out[cellCount * geneCount] doubles.  Returns 0, or 1 for a method the switch does not know ("Invalid normalization method.").
int em2r_dense_expression(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneCount, int method, double* out,
                          double* seconds)
{
    const auto begin = std::chrono::steady_clock::now();
    // the subset's cellExpressionCounts and sums
    std::vector<Sum> sums(cellCount);
    for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
        Sum& sum = sums[cellId];
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) {
            const float& count = data[p].count;
            sum.sum1 += count;
            sum.sum2 += count * count;                 // a float product, widened when it is added
        }
    }

    std::vector<double> dense(size_t(geneCount) * size_t(cellCount), 0.);
    for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
        float normalizationFactor;
        switch (method) {
        case 0:
            normalizationFactor = 1.;
            break;
        case 1:
            normalizationFactor = float(1. / sums[cellId].sum1);
            break;
        case 2:
            normalizationFactor = float(1. / std::sqrt(sums[cellId].sum2));
            break;
        default:
            return 1;
        }
        const size_t offset = size_t(cellId) * size_t(geneCount);
        for (uint64_t p = toc[cellId]; p < toc[cellId + 1]; p++) {
            const std::pair<uint32_t, float> entry(data[p].gene, data[p].count);
            const uint32_t geneId = entry.first;
            float count = normalizationFactor * entry.second;
            dense[offset + geneId] = double(count);
        }
    }
    std::copy(dense.begin(), dense.end(), out);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    return 0;
}

// out holds n ids at least; returns the number kept.
uint64_t em2r_deduplicate(const uint32_t* ids, uint64_t n, uint32_t* out)
{
    std::vector<uint32_t> v(ids, ids + n);
    std::sort(v.begin(), v.end());
    v.resize(std::unique(v.begin(), v.end()) - v.begin());
    std::copy(v.begin(), v.end(), out);
    return v.size();
}

// operation 0: std::set_union, 1: std::set_intersection, 2: std::set_difference of two sorted sets; out holds na + nb ids.
uint64_t em2r_set_operation(int operation, const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, uint32_t* out)
{
    std::vector<uint32_t> result;
    if (operation == 0) std::set_union(a, a + na, b, b + nb, std::back_inserter(result));
    else if (operation == 1) std::set_intersection(a, a + na, b, b + nb, std::back_inserter(result));
    else std::set_difference(a, a + na, b, b + nb, std::back_inserter(result));
    std::copy(result.begin(), result.end(), out);
    return result.size();
}

// out holds n ids; returns the number kept.  seed is the reference's int.
uint64_t em2r_downsample(const uint32_t* input, uint64_t n, double probability, int seed, uint32_t* out)
{
    std::mt19937 randomSource(seed);
    std::vector<uint32_t> kept;
    for (uint64_t i = 0; i < n; i++) {
        const double uniform = double(randomSource()) * (1. / 4294967296.);
        if (uniform < probability) kept.push_back(input[i]);
    }
    std::copy(kept.begin(), kept.end(), out);
    return kept.size();
}

}  // extern "C"
