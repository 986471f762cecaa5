// em2_fsp6.hip -- findSimilarPairs6 on gfx950, bit-identical to src/ExpressionMatrixLsh.cpp:842-1145 (the Charikar
// permutation search, src/charikar.hpp; M. Charikar 2002, section 5).
//
// Reference: one std::mt19937 seeded with the int seed draws permutationCount bit permutations (iota + std::shuffle over
// all lshCount bits, truncated to permutedBitCount, :926-930).  For each permutation the cells are sorted by their
// permuted prefixes (permutedWordCount words, first bit most significant, BitSet.hpp:140-150), ties by cell id (:954,
// std::pair's operator<).  For each cell a std::priority_queue of pointers ordered by prefixLength only (charikar.hpp)
// receives, permutation by permutation, a forward pointer (i+1, if i < cellCount-1) and a backward pointer (i-1, if
// i > 1: the cell at sorted position 1 never starts one, :1031).  searchCount times (or until the queue is empty) the
// top is popped, its cell evaluated (similarityTable[mismatch] > threshold keeps (cell, float similarity)), the
// pointer moved one step and pushed again while it stays in range (:1047-1089).  The kept list is sorted by (float
// similarity desc, id asc), unique'd and cut to k (:1093-1099).
//
// Device formulation:
//   1. permuteKernel: the permuted prefix words of every (permutation, word, cell); the 64 source bits of one output
//      word sit in LDS for the block (the permutations are drawn on the host with libstdc++'s own std::shuffle);
//   2. per permutation a stable rocPRIM radix sort of (word, id) pairs, LSD from the last word to the first, over
//      ascending ids: exactly the reference's total order.  scatterKernel records position[perm][cell] and the
//      prefix words in sorted order;
//   3. walkKernel: one lane per row cell replays the priority queue: libstdc++'s push_heap / __adjust_heap on at most
//      2*permutationCount packed entries (prefixLength:16 | forward:1 | permutation:15 | index:32) in LDS, lane-
//      interleaved.  Each pop evaluates its candidate at once (popcount against the cell's signature) and appends the
//      key (similarity rank << 32 | id) of those above the threshold to the row's list in HBM.  The visit order depends
//      on prefixes only, so this is the whole search;
//   4. selectKernel: one wave per row sorts its list in LDS (bitonic), drops repeated keys (std::unique: the same id
//      always has the same key) and writes the first k.  Rows are processed in chunks that bound the lists' scratch.

#include "em2_device.h"
#include "em2_hip_util.h"
#include "em2_primitives.h"
#include "em2_wave.h"

#include <cstring>

#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

namespace em2 {
namespace {

constexpr uint32_t kMaxPermutations = 64;      // walk: 2*64 entries x 8 B x 64 lanes = 64 KiB of LDS per block
constexpr uint32_t kMaxSearch = 8192;          // select: a list of up to 8192 keys sorts in 64 KiB of LDS
constexpr uint32_t kMaxPrefixWords = 1023;     // prefixLength <= 64 * 1023 fits the entry's 16-bit field
constexpr size_t kListBudget = size_t(1) << 30;

// Packed Charikar pointer.  operator< of charikar.hpp compares prefixLength only: entryLess does the same.
__device__ __forceinline__ uint32_t entryPrefix(uint64_t e) { return uint32_t(e >> 48); }
__device__ __forceinline__ bool entryLess(uint64_t a, uint64_t b) { return entryPrefix(a) < entryPrefix(b); }
__device__ __forceinline__ uint64_t makeEntry(uint32_t prefix, bool forward, uint32_t perm, uint32_t index)
{
    return (uint64_t(prefix) << 48) | (uint64_t(forward ? 1u : 0u) << 47) | (uint64_t(perm) << 32) | index;
}

// grid (cells/256, words, permutations); out[(perm * words + w) * cellCount + cell]
__global__ void __launch_bounds__(256)
permuteKernel(const uint64_t* __restrict__ sig, uint32_t sigWords, uint32_t cellCount, const uint32_t* __restrict__ perms,
              uint32_t permutedBitCount, uint32_t prefixWords, uint64_t* __restrict__ out)
{
    __shared__ uint32_t source[64];
    const uint32_t w = blockIdx.y, p = blockIdx.z;
    const uint32_t first = w * 64u;
    const uint32_t bits = permutedBitCount - first < 64u ? permutedBitCount - first : 64u;
    if (threadIdx.x < bits) source[threadIdx.x] = perms[size_t(p) * permutedBitCount + first + threadIdx.x];
    __syncthreads();
    const uint32_t cell = blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= cellCount) return;
    const uint64_t* row = sig + size_t(cell) * sigWords;
    uint64_t word = 0;
    for (uint32_t j = 0; j < bits; ++j) {                                               // BitSet.hpp:140-150
        const uint32_t s = source[j];
        word |= ((row[s >> 6] >> (63u - (s & 63u))) & 1ull) << (63u - j);
    }
    out[(size_t(p) * prefixWords + w) * cellCount + cell] = word;
}

__global__ void __launch_bounds__(256)
iotaKernel(uint32_t* __restrict__ ids, uint32_t n)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) ids[i] = i;
}

__global__ void __launch_bounds__(256)
gatherWordKernel(const uint64_t* __restrict__ word, const uint32_t* __restrict__ ids, uint32_t n, uint64_t* __restrict__ out)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = word[ids[i]];
}

// position[cell] = i; sorted[i][w] = the prefix words of cellIds[i]
__global__ void __launch_bounds__(256)
scatterKernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ ids, uint32_t n, uint32_t prefixWords,
              uint32_t* __restrict__ position, uint64_t* __restrict__ sorted)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t cell = ids[i];
        position[cell] = i;
        for (uint32_t w = 0; w < prefixWords; ++w) sorted[size_t(i) * prefixWords + w] = words[size_t(w) * n + cell];
    }
}

struct WalkArgs {
    const uint64_t* sig;            // [cellCount][sigWords]
    const uint64_t* permWords;      // [P][prefixWords][cellCount]   prefixes by cell id
    const uint64_t* sortedPrefix;   // [P][cellCount][prefixWords]   prefixes in sorted order
    const uint32_t* cellIds;        // [P][cellCount]
    const uint32_t* position;       // [P][cellCount]
    const uint32_t* keyOfMismatch;  // [lshCount+1]
    uint32_t sigWords, cellCount, permutationCount, searchCount, prefixWords, listCapacity;
    int32_t mGlobal;                // largest mismatch with similarityTable[m] > threshold, -1 if none
};

// BitSet.hpp:294-312
__device__ __forceinline__ uint32_t commonPrefix(const WalkArgs& a, uint32_t p, uint32_t row, uint32_t index)
{
    const uint64_t* mine = a.permWords + size_t(p) * a.prefixWords * a.cellCount + row;
    const uint64_t* theirs = a.sortedPrefix + (size_t(p) * a.cellCount + index) * a.prefixWords;
    uint32_t length = 0;
    for (uint32_t w = 0; w < a.prefixWords; ++w) {
        const uint64_t x = mine[size_t(w) * a.cellCount] ^ theirs[w];
        if (x == 0) {
            length += 64u;
        } else {
            length += uint32_t(__builtin_clzll(x));
            break;
        }
    }
    return length;
}

// libstdc++ std::push_heap (bits/stl_heap.h __push_heap) with std::less on the pointer: the hole rises while its parent
// compares less than the value.  EM2_HEAP(i) is entry i of this lane's heap.
#define EM2_HEAP(i) heap[size_t(i) * 64u + lane]

__device__ __forceinline__ void pushHeap(uint64_t* heap, uint32_t lane, uint32_t hole, uint32_t top, uint64_t value)
{
    uint32_t parent = (hole - 1u) / 2u;
    while (hole > top && entryLess(EM2_HEAP(parent), value)) {
        EM2_HEAP(hole) = EM2_HEAP(parent);
        hole = parent;
        parent = (hole - 1u) / 2u;
    }
    EM2_HEAP(hole) = value;
}

// std::pop_heap on [0, size): the last entry is moved into the hole left by the top (__pop_heap + __adjust_heap).
__device__ __forceinline__ void popHeap(uint64_t* heap, uint32_t lane, uint32_t size)
{
    if (size <= 1u) return;
    const uint32_t len = size - 1u;
    const uint64_t value = EM2_HEAP(len);
    EM2_HEAP(len) = EM2_HEAP(0);
    uint32_t hole = 0, child = 0;
    while (child < (len - 1u) / 2u) {
        child = 2u * (child + 1u);
        if (entryLess(EM2_HEAP(child), EM2_HEAP(child - 1u))) child--;
        EM2_HEAP(hole) = EM2_HEAP(child);
        hole = child;
    }
    if ((len & 1u) == 0u && child == (len - 2u) / 2u) {
        child = 2u * (child + 1u);
        EM2_HEAP(hole) = EM2_HEAP(child - 1u);
        hole = child - 1u;
    }
    pushHeap(heap, lane, hole, 0u, value);
}

// One lane per row of [rowBegin, rowEnd); lists[(row - rowBegin) * listCapacity ...], listCount[row - rowBegin].
__global__ void __launch_bounds__(64)
walkKernel(WalkArgs a, uint32_t rowBegin, uint32_t rowEnd, uint64_t* __restrict__ lists, uint32_t* __restrict__ listCount)
{
    extern __shared__ uint64_t heap[];                         // [2P][64], entry i of lane l at i*64 + l
    const uint32_t lane = threadIdx.x;
    const uint32_t row = rowBegin + blockIdx.x * 64u + lane;
    if (row >= rowEnd) return;
    const uint32_t n = a.cellCount;
    uint32_t size = 0;
    for (uint32_t p = 0; p < a.permutationCount; ++p) {                                 // :1019-1043
        const uint32_t i = a.position[size_t(p) * n + row];
        if (i < n - 1u) {
            pushHeap(heap, lane, size, 0u, makeEntry(commonPrefix(a, p, row, i + 1u), true, p, i + 1u));
            ++size;
        }
        if (i > 1u) {
            pushHeap(heap, lane, size, 0u, makeEntry(commonPrefix(a, p, row, i - 1u), false, p, i - 1u));
            ++size;
        }
    }
    const uint64_t* mine = a.sig + size_t(row) * a.sigWords;
    uint64_t* list = lists + size_t(row - rowBegin) * a.listCapacity;
    uint32_t count = 0;
    for (uint32_t iteration = 0; iteration < a.searchCount && size > 0u; ++iteration) { // :1049-1089
        const uint64_t top = EM2_HEAP(0);
        popHeap(heap, lane, size);
        --size;
        const uint32_t p = uint32_t(top >> 32) & 0x7fffu;
        const bool forward = ((top >> 47) & 1ull) != 0ull;
        uint32_t index = uint32_t(top);
        const uint32_t other = a.cellIds[size_t(p) * n + index];
        const uint64_t* theirs = a.sig + size_t(other) * a.sigWords;
        uint32_t m = 0;
        for (uint32_t w = 0; w < a.sigWords; ++w) m += uint32_t(__builtin_popcountll(mine[w] ^ theirs[w]));
        if (int32_t(m) <= a.mGlobal) list[count++] = (uint64_t(a.keyOfMismatch[m]) << 32) | other;
        bool again = false;
        if (forward) {
            if (index < n - 1u) { ++index; again = true; }
        } else {
            if (index > 0u) { --index; again = true; }
        }
        if (again) {
            pushHeap(heap, lane, size, 0u, makeEntry(commonPrefix(a, p, row, index), forward, p, index));
            ++size;
        }
    }
    listCount[row - rowBegin] = count;
}

#undef EM2_HEAP

// One wave per row: sort the row's keys (bitonic, in LDS), unique, first k.
__global__ void __launch_bounds__(64)
selectKernel(const uint64_t* __restrict__ lists, const uint32_t* __restrict__ listCount, uint32_t listCapacity,
             uint32_t chunkRows, const float* __restrict__ keySimilarity, uint32_t k, PairOut* __restrict__ outPairs,
             uint32_t* __restrict__ outUsed)
{
    extern __shared__ uint64_t keys[];
    const uint32_t lane = threadIdx.x;
    const uint32_t local = blockIdx.x;
    if (local >= chunkRows) return;
    const uint32_t count = listCount[local];
    const uint64_t* list = lists + size_t(local) * listCapacity;
    uint32_t span = 1;
    while (span < count) span <<= 1;
    for (uint32_t i = lane; i < span; i += 64u) keys[i] = i < count ? list[i] : ~0ull;
    __syncthreads();
    for (uint32_t size = 2; size <= span; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            for (uint32_t i = lane; i < span; i += 64u) {
                const uint32_t j = i ^ stride;
                if (j > i) {
                    const uint64_t x = keys[i], y = keys[j];
                    const bool ascending = (i & size) == 0u;
                    if ((x > y) == ascending) {
                        keys[i] = y;
                        keys[j] = x;
                    }
                }
            }
            __syncthreads();
        }
    }
    // :1095-1099: sort (similarity desc, id asc) == key asc; unique; resize(k)
    PairOut* out = outPairs + size_t(local) * k;
    uint32_t kept = 0;
    for (uint32_t base = 0; base < count && kept < k; base += 64u) {
        const uint32_t i = base + lane;
        bool fresh = false;
        uint64_t key = 0;
        if (i < count) {
            key = keys[i];
            fresh = i == 0u || keys[i - 1u] != key;
        }
        const uint64_t mask = __builtin_amdgcn_ballot_w64(fresh);
        const uint32_t rank = kept + lanesBelow(mask);
        if (fresh && rank < k) {
            PairOut po;
            po.cell = uint32_t(key);
            po.similarity = keySimilarity[uint32_t(key >> 32)];
            out[rank] = po;
        }
        kept += uint32_t(__builtin_popcountll(mask));
    }
    if (kept > k) kept = k;
    clearRowTail(out, kept, k, lane);
    if (lane == 0u) outUsed[local] = kept;
}

}  // namespace

uint32_t fsp6MaxPermutations() { return kMaxPermutations; }
uint32_t fsp6MaxSearch() { return kMaxSearch; }
uint32_t fsp6MaxPermutedBits() { return kMaxPrefixWords * 64u; }

uint64_t fsp6EffectiveSearch(uint32_t cellCount, uint32_t permutationCount, uint32_t searchCount)
{
    // the two pointers of a permutation together visit at most the cellCount-1 other cells: the queue is empty then
    const uint64_t most = uint64_t(permutationCount) * (cellCount ? cellCount - 1u : 0u);
    return std::min<uint64_t>(searchCount, most);
}

void fsp6Permutations(uint32_t lshCount, uint32_t permutationCount, uint32_t permutedBitCount, int32_t seed,
                      std::vector<uint32_t>& out)
{
    // :926-930: one generator for all permutations; the shuffle always runs over all lshCount bits
    std::mt19937 randomGenerator(seed);
    out.resize(size_t(permutationCount) * permutedBitCount);
    std::vector<uint64_t> bitPermutation(lshCount);
    for (uint32_t p = 0; p < permutationCount; ++p) {
        std::iota(bitPermutation.begin(), bitPermutation.end(), 0ULL);
        std::shuffle(bitPermutation.begin(), bitPermutation.end(), randomGenerator);
        for (uint32_t i = 0; i < permutedBitCount; ++i) out[size_t(p) * permutedBitCount + i] = uint32_t(bitPermutation[i]);
    }
}

// Arguments validated by the caller (permutationCount <= fsp6MaxPermutations(), 1 <= permutedBitCount <= lshCount,
// permutedBitCount <= fsp6MaxPermutedBits(), fsp6EffectiveSearch() <= fsp6MaxSearch()).  Allocates its own scratch,
// synchronises.
hipError_t runFsp6(const uint64_t* d_sig, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t lshCount, uint32_t k,
                   uint32_t permutationCount, uint32_t searchCount, uint32_t permutedBitCount, int32_t seed,
                   const DeviceTables& tables, PairOut* d_pairs, uint32_t* d_used, hipStream_t stream)
{
    const uint32_t rowCount = rowEnd - rowBegin;
    if (rowCount == 0) return hipSuccess;
    const uint64_t listCapacity64 = fsp6EffectiveSearch(cellCount, permutationCount, searchCount);
    if (permutationCount > kMaxPermutations || listCapacity64 > kMaxSearch || permutedBitCount == 0 ||
        permutedBitCount > lshCount || permutedBitCount > kMaxPrefixWords * 64u) {
        return hipErrorInvalidValue;
    }
    EM2_TRY(hipMemsetAsync(d_used, 0, size_t(rowCount) * sizeof(uint32_t), stream));
    if (k) EM2_TRY(hipMemsetAsync(d_pairs, 0, size_t(rowCount) * k * sizeof(PairOut), stream));
    if (k == 0 || listCapacity64 == 0 || tables.mGlobal < 0) return hipStreamSynchronize(stream);
    const uint32_t listCapacity = uint32_t(listCapacity64);
    const uint32_t sigWords = wordCountOf(lshCount);
    const uint32_t prefixWords = wordCountOf(permutedBitCount);
    const uint32_t n = cellCount;
    const size_t P = permutationCount;

    std::vector<uint32_t> perms;
    fsp6Permutations(lshCount, permutationCount, permutedBitCount, seed, perms);
    DeviceBuffer dPerms, permWords, sortedPrefix, cellIds, position;
    EM2_TRY(dPerms.allocate(perms.size() * sizeof(uint32_t)));
    EM2_TRY(hipMemcpyAsync(dPerms.p, perms.data(), perms.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    EM2_TRY(permWords.allocate(P * prefixWords * n * sizeof(uint64_t)));
    EM2_TRY(sortedPrefix.allocate(P * prefixWords * n * sizeof(uint64_t)));
    EM2_TRY(cellIds.allocate(P * n * sizeof(uint32_t)));
    EM2_TRY(position.allocate(P * n * sizeof(uint32_t)));
    permuteKernel<<<dim3((n + 255u) / 256u, prefixWords, permutationCount), 256, 0, stream>>>(
        d_sig, sigWords, n, dPerms.as<uint32_t>(), permutedBitCount, prefixWords, permWords.as<uint64_t>());
    EM2_TRY(hipGetLastError());

    // :932-1003: sort each permutation's (prefix words, id) pairs; LSD passes, each stable, the first over ascending ids
    {
        DeviceBuffer keysIn, keysOut, idsIn, temp;
        EM2_TRY(keysIn.allocate(size_t(n) * sizeof(uint64_t)));
        EM2_TRY(keysOut.allocate(size_t(n) * sizeof(uint64_t)));
        EM2_TRY(idsIn.allocate(size_t(n) * sizeof(uint32_t)));
        size_t tempBytes = 0;
        EM2_TRY(sortPairsU64U32Bytes(size_t(n), 0u, 64u, tempBytes));
        EM2_TRY(temp.allocate(tempBytes));
        for (uint32_t p = 0; p < permutationCount; ++p) {
            const uint64_t* words = permWords.as<uint64_t>() + size_t(p) * prefixWords * n;
            uint32_t* ids = cellIds.as<uint32_t>() + size_t(p) * n;
            iotaKernel<<<gridFor(n), 256, 0, stream>>>(ids, n);
            EM2_TRY(hipGetLastError());
            for (uint32_t w = prefixWords; w-- > 0;) {
                gatherWordKernel<<<gridFor(n), 256, 0, stream>>>(words + size_t(w) * n, ids, n, keysIn.as<uint64_t>());
                EM2_TRY(hipGetLastError());
                EM2_TRY(hipMemcpyAsync(idsIn.p, ids, size_t(n) * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
                // All 64 bits, the last word's included (its bits after permutedBitCount are zero).  Sorting only that
                // word's live high bits (begin_bit > 0) gave a wrong order from a few thousand cells on.
                EM2_TRY(sortPairs(temp.p, tempBytes, keysIn.as<uint64_t>(), keysOut.as<uint64_t>(), idsIn.as<uint32_t>(), ids, size_t(n), 0u, 64u,
                                  stream));
            }
            scatterKernel<<<gridFor(n), 256, 0, stream>>>(words, ids, n, prefixWords, position.as<uint32_t>() + size_t(p) * n,
                                                            sortedPrefix.as<uint64_t>() + size_t(p) * n * prefixWords);
            EM2_TRY(hipGetLastError());
        }
        EM2_TRY(hipStreamSynchronize(stream));
    }

    // :1005-1100, rows in chunks: the candidate lists take listCapacity keys per row
    uint32_t chunk = uint32_t(std::min<uint64_t>(rowCount, std::max<uint64_t>(64u, kListBudget / (uint64_t(listCapacity) * 8u))));
    DeviceBuffer lists, counts;
    EM2_TRY(lists.allocate(size_t(chunk) * listCapacity * sizeof(uint64_t)));
    EM2_TRY(counts.allocate(size_t(chunk) * sizeof(uint32_t)));
    WalkArgs args;
    args.sig = d_sig;
    args.permWords = permWords.as<uint64_t>();
    args.sortedPrefix = sortedPrefix.as<uint64_t>();
    args.cellIds = cellIds.as<uint32_t>();
    args.position = position.as<uint32_t>();
    args.keyOfMismatch = tables.keyOfMismatch;
    args.sigWords = sigWords;
    args.cellCount = n;
    args.permutationCount = permutationCount;
    args.searchCount = listCapacity;
    args.prefixWords = prefixWords;
    args.listCapacity = listCapacity;
    args.mGlobal = tables.mGlobal;
    const size_t heapBytes = std::max<size_t>(8u, 2u * P * 64u * sizeof(uint64_t));
    uint32_t span = 1;
    while (span < listCapacity) span <<= 1;
    const size_t selectBytes = size_t(span) * sizeof(uint64_t);
    for (uint32_t begin = rowBegin; begin < rowEnd; begin += chunk) {
        const uint32_t end = rowEnd - begin < chunk ? rowEnd : begin + chunk;
        const uint32_t rows = end - begin;
        walkKernel<<<(rows + 63u) / 64u, 64, heapBytes, stream>>>(args, begin, end, lists.as<uint64_t>(), counts.as<uint32_t>());
        EM2_TRY(hipGetLastError());
        selectKernel<<<rows, 64, selectBytes, stream>>>(lists.as<uint64_t>(), counts.as<uint32_t>(), listCapacity, rows,
                                                        tables.keySimilarity, k, d_pairs + size_t(begin - rowBegin) * k,
                                                        d_used + (begin - rowBegin));
        EM2_TRY(hipGetLastError());
    }
    return hipStreamSynchronize(stream);
}

}  // namespace em2
