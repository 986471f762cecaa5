// em2_graph_compare_host_main.cpp -- a stand-alone program around the host-only ends of csrc/em2_graph_compare.hip (the merge
// of the two lists of histogram bins, the fold of the group contingency table over its diagonal, the greedy colouring), for
// a sanitizer build on the CPU (never loaded into Python, never run on a GPU):
//
//   g++ -std=c++17 -g -O1 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o /tmp/em2_graph_compare_host_main tests/native/em2_graph_compare_host_main.cpp
//   /tmp/em2_graph_compare_host_main
//
// Every result is checked against a statement with std::map / std::set written here; the program prints "ok" and returns 0.
#include "../../expressionmatrix2_amd/csrc/em2_graph_compare_host.h"

#include <cstdio>
#include <cstdlib>
#include <limits>
#include <map>
#include <random>
#include <set>
#include <utility>

namespace {

void require(bool condition, const char* what)
{
    if (condition) return;
    fprintf(stderr, "FAILED: %s\n", what);
    exit(1);
}

// Random products: most within the table, some beyond it, both zeros, both infinities.
void checkBins(std::mt19937& random, bool useTable)
{
    const float infinity = std::numeric_limits<float>::infinity();
    std::map<float, uint64_t> expected;                          // (the two zeros are one key; the first one inserted stays)
    std::vector<uint64_t> table(em2::kCompareTableBins, 0u);
    std::map<float, uint64_t> list;
    const int n = int(random() % 300u);
    for (int i = 0; i < n; i++) {
        float r = float(int(random() % 6000u) - 3000);
        const uint32_t kind = random() % 40u;
        if (kind == 0u) r = infinity;
        if (kind == 1u) r = -infinity;
        if (kind == 2u) r = -0.0f;
        if (kind == 3u) r = 0.0f;
        const float product = 0.01f * r;
        expected.insert(std::make_pair(product, uint64_t(0))).first->second++;
        if (useTable && r >= -float(em2::kCompareTableRadius) && r <= float(em2::kCompareTableRadius)) {
            table[size_t(int(r) + em2::kCompareTableRadius)]++;
        } else {
            list[product == 0.0f ? 0.0f : product]++;
        }
    }
    std::vector<float> listDelta, binDelta;
    std::vector<uint64_t> listCount, binCount;
    for (const auto& p : list) {
        listDelta.push_back(p.first);
        listCount.push_back(p.second);
    }
    const auto zero = expected.find(0.0f);
    const bool zeroNegative = zero != expected.end() && (em2::floatBits(zero->first) >> 31) != 0u;
    em2::mergeCompareBins(useTable ? table.data() : nullptr, listDelta, listCount, zeroNegative, binDelta, binCount);
    require(binDelta.size() == expected.size() && binCount.size() == expected.size(), "the number of bins");
    size_t at = 0;
    for (const auto& p : expected) {
        require(em2::floatBits(binDelta[at]) == em2::floatBits(p.first), "a bin's delta, bit for bit");
        require(binCount[at] == p.second, "a bin's count");
        at++;
    }
}

void checkColors(std::mt19937& random)
{
    const uint32_t groupCount = random() % 40u;
    const int cells = groupCount ? int(random() % 400u) : 0;
    std::vector<uint32_t> i0, i1;
    std::vector<uint64_t> count;
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> table;     // the sparse contingency table, ascending
    for (int c = 0; c < cells; c++) table[std::make_pair(uint32_t(random() % groupCount), uint32_t(random() % groupCount))] += 1u + random() % 5u;
    for (const auto& p : table) {
        i0.push_back(p.first.first);
        i1.push_back(p.first.second);
        count.push_back(p.second);
    }
    std::vector<uint32_t> pair0, pair1, colorTable;
    std::vector<uint64_t> pairEdges;
    em2::foldGroupPairs(i0, i1, count, pair0, pair1, pairEdges);
    std::map<std::pair<uint32_t, uint32_t>, uint64_t> folded;
    std::vector<std::set<uint32_t> > adjacency(groupCount);
    for (const auto& p : table) {
        if (p.first.first == p.first.second) continue;
        folded[std::make_pair(std::min(p.first.first, p.first.second), std::max(p.first.first, p.first.second))] += p.second;
        adjacency[p.first.first].insert(p.first.second);
        adjacency[p.first.second].insert(p.first.first);
    }
    require(pair0.size() == folded.size() && pair1.size() == folded.size() && pairEdges.size() == folded.size(), "the number of pairs");
    size_t at = 0;
    for (const auto& p : folded) {
        require(pair0[at] == p.first.first && pair1[at] == p.first.second && pairEdges[at] == p.second, "a pair of groups");
        at++;
    }
    em2::assignGroupColors(groupCount, pair0, pair1, colorTable);
    require(colorTable.size() == groupCount, "a colour per group");
    for (uint32_t g = 0; g < groupCount; g++) {
        std::set<uint32_t> taken;
        for (const uint32_t other : adjacency[g]) {
            if (other < g) taken.insert(colorTable[other]);
        }
        uint32_t color = 0;
        while (taken.count(color)) color++;
        require(colorTable[g] == color, "the smallest colour no smaller neighbour has");
    }
}

}  // namespace

int main()
{
    std::mt19937 random(231);
    for (int trial = 0; trial < 400; trial++) {
        checkBins(random, trial % 2 == 0);
        checkColors(random);
    }
    // nothing at all
    std::vector<float> binDelta;
    std::vector<uint64_t> binCount;
    em2::mergeCompareBins(nullptr, std::vector<float>(), std::vector<uint64_t>(), false, binDelta, binCount);
    require(binDelta.empty() && binCount.empty(), "no bins");
    std::vector<uint32_t> colorTable;
    em2::assignGroupColors(3, std::vector<uint32_t>(), std::vector<uint32_t>(), colorTable);
    require(colorTable == std::vector<uint32_t>(3, 0u), "groups without pairs share colour 0");
    printf("ok\n");
    return 0;
}
