// em2_rank_genes_host.h -- the statistics of the rank-sum (Mann-Whitney / Wilcoxon) test of one gene for one group against the
// rest, from the integers em2_rank_genes.hip counts.  Host code without HIP, so that the library, the
// one-thread restatement of the tests and a stand-alone program under a sanitizer compile the same lines.
//
// The inputs are exact integers: N cells, n of them in the group, rankSum2 = the sum over the group's cells of TWICE the
// mid-rank of the cell's value among all N (ranks from 1), tieSum = the sum of t^3 - t over the tie groups of the N values.
// N <= 2^21 (kRankGenesMaxCells), so every integer expression below stays within 64 bits.
//
// The order of the operations, each double operation rounded once (no FMA: -ffp-contract=off):
//   m    = N - n                                         integer
//   u2   = rankSum2 - n * (n + 1)                        integer, twice the U statistic of the group; never negative
//   num  = u2 - n * m                                    integer (int64), twice (U - n m / 2)
//   s    = N * N * N - N - tieSum                        integer
//   var  = ((double(n) * double(m)) * double(s)) / ((12. * double(N)) * double(N - 1))
//   z    = (0.5 * double(num)) / sqrt(var)               0 where var is not positive (an empty group, a group that is the whole
//                                                        universe, one tie group of N values, N = 1 where var is 0 / 0)
//   auc  = double(u2) / ((2. * double(n)) * double(m))   0.5 where n * m = 0
// There is no continuity correction.  The two-sided p-value of the normal approximation is erfc(|z| / sqrt(2)).
#ifndef EM2_RANK_GENES_HOST_H
#define EM2_RANK_GENES_HOST_H

#include <cmath>
#include <cstdint>

namespace em2 {

constexpr uint64_t kRankGenesMaxCells = 1ull << 21;        // above it t^3 leaves 64 bits and 2 N^2 leaves 2^53

struct RankGeneStatistics {
    double zScore, auc;
};

inline RankGeneStatistics rankGeneStatistics(uint64_t cellCount, uint64_t groupSize, uint64_t rankSum2, uint64_t tieSum)
{
    const uint64_t N = cellCount, n = groupSize, m = N - n;
    const uint64_t u2 = rankSum2 - n * (n + 1u);
    const int64_t num = int64_t(u2) - int64_t(n * m);
    const uint64_t s = N * N * N - N - tieSum;
    const double nm = double(n) * double(m);
    const double var = (nm * double(s)) / ((12. * double(N)) * double(N - 1u));
    RankGeneStatistics out;
    out.zScore = var > 0. ? (0.5 * double(num)) / std::sqrt(var) : 0.;
    out.auc = n * m != 0u ? double(u2) / ((2. * double(n)) * double(m)) : 0.5;
    return out;
}

// zScore[gene * groupCount + group] and auc likewise, from the arrays of em2_rank_genes.
inline void rankGeneStatisticsOfAll(uint64_t cellCount, uint32_t geneCount, uint32_t groupCount, const uint32_t* groupSize,
                                    const uint64_t* rankSum2, const uint64_t* tieSum, double* zScore, double* auc)
{
    for (uint64_t g = 0; g < geneCount; ++g) {
        for (uint64_t k = 0; k < groupCount; ++k) {
            const RankGeneStatistics s = rankGeneStatistics(cellCount, groupSize[k], rankSum2[g * groupCount + k], tieSum[g]);
            if (zScore) zScore[g * groupCount + k] = s.zScore;
            if (auc) auc[g * groupCount + k] = s.auc;
        }
    }
}

}  // namespace em2

#endif
