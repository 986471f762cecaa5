// em2_rank_genes_host_main.cpp -- a stand-alone program around the statistics of the rank-sum test
// (csrc/em2_rank_genes_host.h), for a sanitizer build on the CPU (never loaded into Python, never run on a GPU):
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o /tmp/em2_rank_genes_host_main tests/native/em2_rank_genes_host_main.cpp
//   /tmp/em2_rank_genes_host_main
//
// It runs the header over its edge cases -- an empty group, a group that is the whole universe, one cell, one tie group of all
// values, the largest supported universe (2^21 cells, where N^3 and the rank sums are closest to 64 bits), a perfect
// separation in both directions -- and over a small example worked out by hand; it prints "rank genes host checks ok" and
// returns 0, or says what failed and returns 1.
#include "../../expressionmatrix2_amd/csrc/em2_rank_genes_host.h"

#include <cmath>
#include <cstdio>
#include <vector>

namespace {

int failures = 0;

void expect(bool condition, const char* what)
{
    if (!condition) {
        std::printf("FAILED: %s\n", what);
        ++failures;
    }
}

}  // namespace

int main()
{
    using em2::rankGeneStatistics;
    // an empty group: rankSum2 = 0, n m = 0
    em2::RankGeneStatistics s = rankGeneStatistics(10, 0, 0, 0);
    expect(s.zScore == 0. && !std::signbit(s.zScore) && s.auc == 0.5, "an empty group gives z = 0, auc = 0.5");
    // the whole universe: rankSum2 = N (N + 1)
    s = rankGeneStatistics(10, 10, 110, 0);
    expect(s.zScore == 0. && s.auc == 0.5, "the whole universe gives z = 0, auc = 0.5");
    // one cell: the variance is 0 / 0
    s = rankGeneStatistics(1, 1, 2, 0);
    expect(s.zScore == 0. && s.auc == 0.5, "one cell in its group gives z = 0, auc = 0.5");
    s = rankGeneStatistics(1, 0, 0, 0);
    expect(s.zScore == 0. && s.auc == 0.5, "one cell in no group gives z = 0, auc = 0.5");
    // one tie group of all N values: every mid-rank is (N + 1) / 2, tieSum = N^3 - N, no variance
    s = rankGeneStatistics(10, 4, 4 * 11, 990);
    expect(s.zScore == 0. && s.auc == 0.5, "one tie group of all values gives z = 0, auc = 0.5");
    // by hand: values 1 2 3 4 5, the group holds 4 and 5: ranks 4 + 5, U = 9 - 3 = 6 = n m, var = 2 * 3 * 120 / (12 * 5 * 4) = 3
    s = rankGeneStatistics(5, 2, 18, 0);
    expect(s.auc == 1. && s.zScore == 3. / std::sqrt(3.), "the top two of five: auc = 1, z = 3 / sqrt(3)");
    // the bottom two: ranks 1 + 2, U = 0
    s = rankGeneStatistics(5, 2, 6, 0);
    expect(s.auc == 0. && s.zScore == -3. / std::sqrt(3.), "the bottom two of five: auc = 0, z = -3 / sqrt(3)");
    // with ties: values 0 0 0 1 1, the group holds the two ones: mid-ranks 4.5 each, tieSum = 24 + 6, var = 6 * 90 / 240
    s = rankGeneStatistics(5, 2, 18, 30);
    expect(s.auc == 1. && s.zScore == 3. / std::sqrt(2.25), "the two ones among three zeros: auc = 1, z = 2");
    // the largest universe: N = 2^21, half of it in the group, on top.  rankSum2 = 2 * (sum of the ranks N/2 + 1 .. N).
    const uint64_t N = em2::kRankGenesMaxCells, n = N / 2;
    const uint64_t top = (N * (N + 1) - n * (n + 1));                    // twice the sum of the upper half's ranks
    s = rankGeneStatistics(N, n, top, 0);
    expect(s.auc == 1., "2^21 cells, the upper half: auc = 1");
    const double var = (double(n) * double(n)) * double(N * N * N - N) / ((12. * double(N)) * double(N - 1));
    expect(s.zScore == (0.5 * double(n * n)) / std::sqrt(var) && s.zScore > 1254. && s.zScore < 1255., "2^21 cells, the upper half: z = sqrt(3 N) / 2 nearly");
    s = rankGeneStatistics(N, n, n * (n + 1), 0);
    expect(s.auc == 0. && s.zScore < -1254., "2^21 cells, the lower half: auc = 0");
    s = rankGeneStatistics(N, N, N * (N + 1), N * N * N - N);
    expect(s.zScore == 0. && s.auc == 0.5, "2^21 cells in one tie group and one group");
    // the arrays: [gene][group], either output may be left out
    const uint32_t sizes[2] = {2, 3};
    const uint64_t sums[4] = {18, 12, 6, 24}, ties[2] = {0, 0};
    std::vector<double> z(4, -1.), auc(4, -1.);
    em2::rankGeneStatisticsOfAll(5, 2, 2, sizes, sums, ties, z.data(), nullptr);
    em2::rankGeneStatisticsOfAll(5, 2, 2, sizes, sums, ties, nullptr, auc.data());
    expect(z[0] == -z[1] && z[2] == -z[3] && z[0] == -z[2], "two complementary groups have opposite z");
    expect(auc[0] == 1. && auc[1] == 0. && auc[2] == 0. && auc[3] == 1., "two complementary groups have complementary auc");
    if (failures) return 1;
    std::printf("rank genes host checks ok\n");
    return 0;
}
