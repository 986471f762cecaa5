// em2_rank_genes_restatement.cpp -- the rank-sum test of em2_rank_genes (include/em2_lsh.h) restated for one
// thread from the definition of a mid-rank alone: per gene it gathers the values of ALL cells (+0 where a cell stores nothing),
// sorts them with std::sort, walks the tie groups and adds twice the mid-rank (a + b + 1 for the positions [a, b), ranks from
// 1) to the group of every member.  Nothing of the library's short cuts is here: no rule for the zeros, no run tables, no keys.
// The statistics are those of csrc/em2_rank_genes_host.h, the one header the library, this file and the stand-alone program
// share.  Test infrastructure only.
//
// Build: g++ -std=c++17 -O2 -ffp-contract=off -fPIC -shared (tests/rank_genes_binding.py).
#include "../../expressionmatrix2_amd/csrc/em2_rank_genes_host.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <utility>
#include <vector>

namespace {

struct Count {
    uint32_t gene;
    float count;
};

constexpr uint32_t kNoGroup = 0xffffffffu;

}  // namespace

extern "C" {

// The genes [geneBegin, geneEnd) of the CSR; the outputs are [geneEnd - geneBegin][groupCount] (tieSum [geneEnd - geneBegin],
// groupSize [groupCount]).  Returns 0, or 1 where a value is NaN (nothing is then promised of the outputs).  *seconds: the
// time of the gene loop.
int em2r_rank_genes(const uint64_t* toc, const Count* data, uint32_t cellCount, uint32_t geneBegin, uint32_t geneEnd,
                    const double* normInverse, const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount,
                    uint64_t* rankSum2, uint64_t* tieSum, double* zScore, double* auc, double* seconds)
{
    for (uint32_t k = 0; k < groupCount; ++k) groupSize[k] = 0;
    for (uint32_t c = 0; c < cellCount; ++c) {
        if (group[c] != kNoGroup) ++groupSize[group[c]];
    }
    const auto start = std::chrono::steady_clock::now();
    std::vector<std::pair<float, uint32_t>> values(cellCount);          // (value, group)
    for (uint32_t gene = geneBegin; gene < geneEnd; ++gene) {
        for (uint32_t c = 0; c < cellCount; ++c) {
            float value = 0.f;
            const Count* begin = data + toc[c];
            const Count* end = data + toc[c + 1];
            const Count* at = std::lower_bound(begin, end, gene, [](const Count& e, uint32_t g) { return e.gene < g; });
            if (at != end && at->gene == gene) {
                value = normInverse ? at->count * float(normInverse[c]) : at->count;
                if (value != value) return 1;
                if (value == 0.f) value = 0.f;                           // -0 counts as +0
            }
            values[c] = std::make_pair(value, group[c]);
        }
        std::sort(values.begin(), values.end(), [](const std::pair<float, uint32_t>& x, const std::pair<float, uint32_t>& y) { return x.first < y.first; });
        const size_t row = size_t(gene - geneBegin) * groupCount;
        for (uint32_t k = 0; k < groupCount; ++k) {
            nonZeroCount[row + k] = 0;
            rankSum2[row + k] = 0;
        }
        uint64_t ties = 0;
        for (uint64_t a = 0; a < cellCount;) {
            uint64_t b = a + 1;
            while (b < cellCount && values[b].first == values[a].first) ++b;
            const uint64_t t = b - a;
            ties += t * t * t - t;
            for (uint64_t i = a; i < b; ++i) {
                if (values[i].second == kNoGroup) continue;
                rankSum2[row + values[i].second] += a + b + 1;         // twice ((a + 1) + b) / 2
                if (values[i].first != 0.f) ++nonZeroCount[row + values[i].second];
            }
            a = b;
        }
        tieSum[gene - geneBegin] = ties;
    }
    *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - start).count();
    em2::rankGeneStatisticsOfAll(cellCount, geneEnd - geneBegin, groupCount, groupSize, rankSum2, tieSum, zScore, auc);
    return 0;
}

}  // extern "C"
