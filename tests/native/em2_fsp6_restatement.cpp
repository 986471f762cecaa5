// em2_fsp6_restatement.cpp -- TEST-ONLY literal C++ restatement of ExpressionMatrix::findSimilarPairs6
// (src/ExpressionMatrixLsh.cpp:842-1145, src/charikar.hpp, src/BitSet.hpp), written from the reference's contract with the
// same standard-library pieces it uses: std::mt19937, std::shuffle, std::sort, std::priority_queue, std::unique.  It is
// compiled with the host's g++ at test time (tests/fsp6_binding.py), so its shuffle and its heap are the libstdc++ of the
// box the tests run on -- which is the contract.  The GPU path (expressionmatrix2_amd/csrc/em2_fsp6.hip) is checked
// against it; nothing here is shipped or used by the product.

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <queue>
#include <random>
#include <utility>
#include <vector>

namespace {

// src/charikar.hpp: Charikar::Pointer, ordered by prefixLength only.
struct Pointer {
    size_t permutationId;
    size_t index;
    bool movesForward;
    size_t prefixLength;
    bool operator<(const Pointer& that) const { return prefixLength < that.prefixLength; }
};

// Lsh.cpp:229-249 (pi: the double nearest to pi)
std::vector<double> similarityTable(uint32_t lshCount)
{
    const double pi = 3.141592653589793238462643383279502884;
    std::vector<double> table(size_t(lshCount) + 1);
    for (size_t m = 0; m <= lshCount; m++) table[m] = std::cos(double(m) * pi / double(lshCount));
    return table;
}

// :926-930: one generator, seeded once with the int seed; each permutation shuffles all lshCount bits and keeps the
// first permutedBitCount.
void drawPermutations(uint32_t lshCount, uint32_t permutationCount, uint32_t permutedBitCount, int32_t seed,
                      std::vector<std::vector<uint64_t>>& out)
{
    std::mt19937 randomGenerator(seed);
    out.assign(permutationCount, std::vector<uint64_t>());
    for (uint32_t p = 0; p < permutationCount; p++) {
        std::vector<uint64_t> bitPermutation(lshCount);
        std::iota(bitPermutation.begin(), bitPermutation.end(), 0ULL);
        std::shuffle(bitPermutation.begin(), bitPermutation.end(), randomGenerator);
        bitPermutation.resize(permutedBitCount);
        out[p] = bitPermutation;
    }
}

// BitSet.hpp:294-312
size_t commonPrefixLength(const uint64_t* x, const uint64_t* y, size_t wordCount)
{
    size_t prefixLength = 0;
    for (size_t i = 0; i < wordCount; i++) {
        if (x[i] == y[i]) {
            prefixLength += 64;
        } else {
            prefixLength += size_t(__builtin_clzll(x[i] ^ y[i]));
            break;
        }
    }
    return prefixLength;
}

}  // namespace

extern "C" {

// The permutations of :926-930, [permutationCount][permutedBitCount].
void em2r_fsp6_permutations(uint32_t lshCount, uint32_t permutationCount, uint32_t permutedBitCount, int32_t seed, uint32_t* out)
{
    std::vector<std::vector<uint64_t>> permutations;
    drawPermutations(lshCount, permutationCount, permutedBitCount, seed, permutations);
    for (uint32_t p = 0; p < permutationCount; p++) {
        for (uint32_t i = 0; i < permutedBitCount; i++) out[size_t(p) * permutedBitCount + i] = uint32_t(permutations[p][i]);
    }
}

// findSimilarPairs6 for the cells rows[0..rowCount) (rows == NULL: every cell, rowCount ignored).  Output row r of
// outCell/outSimilarity ([rowCount][k], zero beyond outUsed[r]) belongs to rows[r].  Returns 0, or 1 when
// permutedBitCount exceeds lshCount (:886-893), 2 when permutedBitCount is 0 (the reference dies there).
int em2r_find_similar_pairs6(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                             double similarityThreshold, uint32_t permutationCount, uint32_t searchCount,
                             uint32_t permutedBitCount, int32_t seed, const uint32_t* rows, uint32_t rowCount,
                             uint32_t* outCell, float* outSimilarity, uint32_t* outUsed)
{
    if (permutedBitCount > lshCount) return 1;
    if (permutedBitCount == 0) return 2;
    const size_t wordCount = (size_t(lshCount) - 1) / 64 + 1;
    const size_t permutedWordCount = ((size_t(permutedBitCount) - 1) >> 6) + 1;              // :920
    const std::vector<double> table = similarityTable(lshCount);
    auto getBit = [&](uint32_t cell, uint64_t bit) -> bool {
        return ((signatures[size_t(cell) * wordCount + (bit >> 6)] >> (63u - (bit & 63u))) & 1ull) != 0;
    };

    // Phase 1 (:932-1003): permuted signatures, sorted by (signature, cell id), and the position of each cell.
    std::vector<std::vector<uint64_t>> permutations;
    drawPermutations(lshCount, permutationCount, permutedBitCount, seed, permutations);
    std::vector<std::vector<uint64_t>> sortedSignatures(permutationCount);    // [permutation][i * permutedWordCount + w]
    std::vector<std::vector<uint32_t>> cellIds(permutationCount);
    std::vector<std::vector<size_t>> cellPositions(permutationCount);
    for (uint32_t p = 0; p < permutationCount; p++) {
        std::vector<uint64_t> permuted(size_t(cellCount) * permutedWordCount, 0ULL);
        for (uint32_t cell = 0; cell < cellCount; cell++) {                                  // fillUsingPermutation
            for (size_t i = 0; i < permutations[p].size(); i++) {
                if (getBit(cell, permutations[p][i])) permuted[cell * permutedWordCount + (i >> 6)] |= 1ull << (63u - (i & 63u));
            }
        }
        std::vector<std::pair<std::vector<uint64_t>, uint32_t>> sorted(cellCount);
        for (uint32_t cell = 0; cell < cellCount; cell++) {
            sorted[cell].first.assign(permuted.begin() + cell * permutedWordCount, permuted.begin() + (cell + 1) * permutedWordCount);
            sorted[cell].second = cell;
        }
        std::sort(sorted.begin(), sorted.end());              // lexicographic words, then cell id (BitSet.hpp:157-160)
        sortedSignatures[p].resize(size_t(cellCount) * permutedWordCount);
        cellIds[p].resize(cellCount);
        cellPositions[p].resize(cellCount);
        for (uint32_t i = 0; i < cellCount; i++) {
            std::copy(sorted[i].first.begin(), sorted[i].first.end(), sortedSignatures[p].begin() + size_t(i) * permutedWordCount);
            cellIds[p][i] = sorted[i].second;
            cellPositions[p][sorted[i].second] = i;                                            // computeCellPositions
        }
    }

    // Phase 2 (:1005-1100), for the requested rows.
    const uint32_t outRows = rows ? rowCount : cellCount;
    std::vector<std::pair<uint32_t, float>> cellNeighbors;
    for (uint32_t r = 0; r < outRows; r++) {
        const uint32_t cellId0 = rows ? rows[r] : r;
        auto signature0 = [&](size_t p) { return sortedSignatures[p].data() + cellPositions[p][cellId0] * permutedWordCount; };
        std::priority_queue<Pointer> priorityQueue;
        for (size_t p = 0; p < permutationCount; p++) {                                       // :1019-1043
            const size_t i = cellPositions[p][cellId0];
            if (i < size_t(cellCount) - 1) {
                Pointer pointer;
                pointer.permutationId = p;
                pointer.index = i + 1;
                pointer.movesForward = true;
                pointer.prefixLength = commonPrefixLength(signature0(p), sortedSignatures[p].data() + (i + 1) * permutedWordCount, permutedWordCount);
                priorityQueue.push(pointer);
            }
            if (i > 1) {                                       // sic: the cell at sorted position 1 gets no backward pointer
                Pointer pointer;
                pointer.permutationId = p;
                pointer.index = i - 1;
                pointer.movesForward = false;
                pointer.prefixLength = commonPrefixLength(signature0(p), sortedSignatures[p].data() + (i - 1) * permutedWordCount, permutedWordCount);
                priorityQueue.push(pointer);
            }
        }
        cellNeighbors.clear();
        for (size_t iteration = 0; iteration < searchCount; iteration++) {                  // :1049-1089
            if (priorityQueue.empty()) break;
            Pointer pointer = priorityQueue.top();
            priorityQueue.pop();
            const uint32_t cellId1 = cellIds[pointer.permutationId][pointer.index];
            size_t mismatchCount = 0;
            for (size_t w = 0; w < wordCount; w++) {
                mismatchCount += size_t(__builtin_popcountll(signatures[size_t(cellId0) * wordCount + w] ^
                                                             signatures[size_t(cellId1) * wordCount + w]));
            }
            const double similarity = table[mismatchCount];
            if (similarity > similarityThreshold) cellNeighbors.push_back(std::make_pair(cellId1, float(similarity)));
            const uint64_t* signature = sortedSignatures[pointer.permutationId].data();
            if (pointer.movesForward) {
                if (pointer.index < size_t(cellCount) - 1) {
                    ++pointer.index;
                    pointer.prefixLength = commonPrefixLength(signature0(pointer.permutationId), signature + pointer.index * permutedWordCount, permutedWordCount);
                    priorityQueue.push(pointer);
                }
            } else {
                if (pointer.index > 0) {
                    --pointer.index;
                    pointer.prefixLength = commonPrefixLength(signature0(pointer.permutationId), signature + pointer.index * permutedWordCount, permutedWordCount);
                    priorityQueue.push(pointer);
                }
            }
        }
        // :1093-1099 (OrderPairsBySecondGreaterThenByFirstLess, orderPairs.hpp:44-52), then SimilarPairs::copy
        std::sort(cellNeighbors.begin(), cellNeighbors.end(),
                  [](const std::pair<uint32_t, float>& x, const std::pair<uint32_t, float>& y) {
                      if (x.second > y.second) return true;
                      if (y.second > x.second) return false;
                      return x.first < y.first;
                  });
        cellNeighbors.resize(size_t(std::unique(cellNeighbors.begin(), cellNeighbors.end()) - cellNeighbors.begin()));
        if (cellNeighbors.size() > k) cellNeighbors.resize(k);
        for (uint32_t j = 0; j < k; j++) {
            const bool used = j < cellNeighbors.size();
            outCell[size_t(r) * k + j] = used ? cellNeighbors[j].first : 0u;
            outSimilarity[size_t(r) * k + j] = used ? cellNeighbors[j].second : 0.0f;
        }
        outUsed[r] = uint32_t(cellNeighbors.size());
    }
    return 0;
}

}  // extern "C"
