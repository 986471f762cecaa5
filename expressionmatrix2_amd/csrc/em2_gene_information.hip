// em2_gene_information.hip -- ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) and the
// count of expressing cells of createWellExpressedGeneSet (src/ExpressionMatrixGeneSets.cpp:336-350) for every gene of a
// subset's CSR in device memory.
//
// The reference walks gene by gene and looks every cell up with a binary search (getCellExpressionCount, :1035-1046).  Here
// the stored entries are transposed once and every gene's entries are reduced where they then lie together:
//   * cellNormInversesKernel   Cell::norm1Inverse / norm2Inverse as addCell defines them (:241-263): walkCell
//                              (em2_expression.h) over the whole row of every cell, a thread per cell;
//   * entriesKernel            a wave per cell: key = local gene, value = c = count * float(normInverse) (a float product,
//                              :1981-1992), in stored order; the gene ids are checked as walkCell checks them; a cell whose
//                              float(normInverse) is not finite raises the `poison` word (see geneSumsKernel);
//   * rocPRIM's STABLE radix sort of (key, value) on the bits a gene id needs: every gene's values together, its cells still in
//     ascending order, so the stream is a function of the input alone;
//   * geneSegmentsKernel       the segment of every gene by binary search on the sorted keys; its length is the number of
//                              expressing cells, stored zeros included; ceil(length / kChunk) chunks;
//   * a scan over the chunk counts and chunkTableKernel (em2_chunks.h): chunk t -> (gene, chunk within the gene).  The work of both passes is
//     dealt by chunk, so a gene present in every cell and a gene present in one cell keep the machine equally busy;
//   * chunkReduceKernel<PASS>  THE FIXED SHAPE.  A gene's segment is cut at kChunk, 2 kChunk, ... FROM ITS OWN START.  One wave
//                              reduces one chunk: lane l adds the chunk's entries l, l + 64, l + 128, ... in ascending order
//                              into a double that starts at +0, then the 64 lane sums are folded by waveSum (em2_wave.h:
//                              lanes l and l ^ 32, then ^ 16, ... ^ 1).  Pass 0 adds double(c); pass 1 adds p * log(p) for
//                              c > 0, p = double(c) * inverseSum(gene).  Which wave of which block reduces a chunk changes nothing;
//   * geneSumsKernel / geneFinishKernel   a thread per gene adds the gene's chunk partials in ascending chunk order:
//                              sum, inverseSum = 1 / sum; then I = (logN + s) / log2, float(I).
// No floating-point atomics, no FMA (-ffp-contract=off), the device library's double log.
//
// A cell whose float(normInverse) is inf or NaN (an empty cell under L1 / L2): the reference multiplies the 0 of every gene
// the cell does not store by it (:1981-1987) and adds the NaN to that gene's sum; a gene the cell does store gets inf or NaN
// there.  Either way every gene with a positive entry ends as NaN and every other gene as log(N) / log(2).  geneSumsKernel
// restates that by replacing every gene's sum with NaN when the poison word is set.

#include "em2_device.h"
#include "em2_expression.h"
#include "em2_entry.h"
#include "em2_csr.h"
#include "em2_chunks.h"
#include "em2_primitives.h"
#include "em2_wave.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <string>

namespace em2 {
namespace {

constexpr uint32_t kChunk = kGeneInformationChunk;       // entries of a gene one wave reduces
constexpr uint32_t kPerLane = kChunk / 64u;

__global__ void __launch_bounds__(256)
cellNormInversesKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
                       int method, double* __restrict__ normInverse)
{
    for (uint64_t c = blockIdx.x * blockDim.x + threadIdx.x; c < cellCount; c += uint64_t(gridDim.x) * blockDim.x) {
        const CellWalk w = walkCell(toc, data, c, geneCount);
        normInverse[c] = method == 1 ? __ddiv_rn(1., w.sum1) : __ddiv_rn(1., __dsqrt_rn(w.sum2));      // :262-263
    }
}

// words[0] |= the input error of walkCell (bit 2: toc does not cover exactly the entryCount entries, from 0 and ascending; such
// a cell writes nothing), words[1] |= 1 where a cell's factor is not finite.  normInverse NULL: no scaling.
__global__ void __launch_bounds__(256)
entriesKernel(const uint64_t* __restrict__ toc, const CountIn* __restrict__ data, uint32_t cellCount, uint32_t geneCount,
              uint64_t entryCount, const double* __restrict__ normInverse, uint32_t* __restrict__ keys, float* __restrict__ values,
              uint32_t* __restrict__ words)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = uint64_t(gridDim.x) * (blockDim.x >> 6);
    uint32_t bad = 0u;
    if (blockIdx.x == 0u && threadIdx.x == 0u && (toc[0] != 0u || toc[cellCount] != entryCount)) bad |= 4u;
    for (uint64_t cell = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); cell < cellCount; cell += waves) {
        const uint64_t begin = toc[cell];
        uint64_t end = toc[cell + 1u];
        if (end > entryCount || begin > end) {                 // (a toc that descends: cells would write each other's entries)
            bad |= 4u;
            end = begin;
        }
        float factor = 1.f;
        if (normInverse) {
            factor = float(normInverse[cell]);
            if (lane == 0u && !(fabsf(factor) <= 3.402823466e38f)) atomicOr(words + 1, 1u);
        }
        for (uint64_t p = begin + lane; p < end; p += 64u) {
            const CountIn e = data[p];
            if (e.gene >= geneCount) bad |= 1u;
            if (p != begin && e.gene <= data[p - 1u].gene) bad |= 2u;
            keys[p] = e.gene;
            values[p] = normInverse ? e.count * factor : e.count;
        }
    }
    if (bad) atomicOr(words, bad);
}

__device__ __forceinline__ uint64_t lowerBound(const uint32_t* __restrict__ sorted, uint64_t count, uint32_t key)
{
    uint64_t low = 0, high = count;
    while (low < high) {
        const uint64_t middle = low + (high - low) / 2u;
        if (sorted[middle] < key) low = middle + 1u;
        else high = middle;
    }
    return low;
}

// offsets[g] = the first entry of gene g in the sorted stream (offsets[geneCount] = count); chunkCounts[g] = its chunks
// (chunkCounts[geneCount] = 0, the scan's last input); expressing[g] (NULL or [geneCount]) = its entries.
__global__ void __launch_bounds__(256)
geneSegmentsKernel(const uint32_t* __restrict__ sortedKeys, uint64_t count, uint32_t geneCount, uint64_t* __restrict__ offsets,
                   uint64_t* __restrict__ chunkCounts, uint32_t* __restrict__ expressing)
{
    for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g <= geneCount; g += uint64_t(gridDim.x) * blockDim.x) {
        if (g == geneCount) {
            offsets[g] = count;
            chunkCounts[g] = 0u;
            continue;
        }
        const uint64_t begin = lowerBound(sortedKeys, count, uint32_t(g));
        const uint64_t end = g + 1u == geneCount ? count : lowerBound(sortedKeys, count, uint32_t(g + 1u));
        offsets[g] = begin;
        chunkCounts[g] = (end - begin + kChunk - 1u) / kChunk;
        if (expressing) expressing[g] = uint32_t(end - begin);
    }
}

// partials[t] for the chunks t = wave, wave + waves, ...  PASS 0: the sum of double(c).  PASS 1: the sum of p * log(p) over c > 0.
template <int PASS>
__global__ void __launch_bounds__(256)
chunkReduceKernel(const float* __restrict__ sortedValues, const uint64_t* __restrict__ offsets, const uint64_t* __restrict__ chunkStarts,
                  uint32_t geneCount, const ChunkRef* __restrict__ table, const double* __restrict__ inverseSums,
                  double* __restrict__ partials)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = uint64_t(gridDim.x) * (blockDim.x >> 6);
    const uint64_t total = chunkStarts[geneCount];
    for (uint64_t t = uint64_t(blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6); t < total; t += waves) {
        const ChunkRef chunk = table[t];
        const uint64_t begin = offsets[chunk.gene] + uint64_t(chunk.index) * kChunk;
        const uint64_t segmentEnd = offsets[chunk.gene + 1u];
        const uint64_t end = begin + kChunk < segmentEnd ? begin + kChunk : segmentEnd;
        const double inverseSum = PASS == 1 ? inverseSums[chunk.gene] : 0.;
        float c[kPerLane];
#pragma unroll
        for (uint32_t i = 0; i < kPerLane; ++i) {
            const uint64_t p = begin + lane + 64u * i;
            c[i] = p < end ? sortedValues[p] : 0.f;                    // (behind the end: +0, no term in either pass)
        }
        double mine = 0.;
#pragma unroll
        for (uint32_t i = 0; i < kPerLane; ++i) {
            const uint64_t p = begin + lane + 64u * i;
            if (PASS == 0) {
                if (p < end) mine += double(c[i]);
            } else if (p < end && c[i] > 0.f) {                         // :2007 (false for NaN)
                const double probability = double(c[i]) * inverseSum;  // :2008
                const double term = probability * log(probability);    // rounded
                mine += term;                                           // rounded again: never an FMA
            }
        }
        const double all = waveSum(mine);
        if (lane == 0u) partials[t] = all;
    }
}

// sums[g] = the gene's chunk partials added in ascending order from +0 (NaN instead where a cell poisons every sum),
// inverseSums[g] = 1 / sums[g] (:2005).
__global__ void __launch_bounds__(256)
geneSumsKernel(const double* __restrict__ partials, const uint64_t* __restrict__ chunkStarts, uint32_t geneCount,
               const uint32_t* __restrict__ words, double* __restrict__ sums, double* __restrict__ inverseSums)
{
    const bool poison = words[1] != 0u;
    for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < geneCount; g += uint64_t(gridDim.x) * blockDim.x) {
        double sum = 0.;
        for (uint64_t t = chunkStarts[g]; t < chunkStarts[g + 1u]; ++t) sum += partials[t];
        if (poison) sum = __longlong_as_double(0x7ff8000000000000ll);
        sums[g] = sum;
        inverseSums[g] = __ddiv_rn(1., sum);
    }
}

// :2004-2017: I = log(N) + the terms, / log(2), float.  logN and log2 are the host's.
__global__ void __launch_bounds__(256)
geneFinishKernel(const double* __restrict__ partials, const uint64_t* __restrict__ chunkStarts, uint32_t geneCount, double logN,
                 double log2, float* __restrict__ informationContent, double* __restrict__ informationContentDouble)
{
    for (uint64_t g = blockIdx.x * blockDim.x + threadIdx.x; g < geneCount; g += uint64_t(gridDim.x) * blockDim.x) {
        double terms = 0.;
        for (uint64_t t = chunkStarts[g]; t < chunkStarts[g + 1u]; ++t) terms += partials[t];
        const double information = __ddiv_rn(logN + terms, log2);
        informationContent[g] = float(information);
        if (informationContentDouble) informationContentDouble[g] = information;
    }
}

uint32_t geneBitsOf(uint32_t geneCount)
{
    uint32_t bits = 0;
    while (bits < 32u && (1ull << bits) < geneCount) ++bits;
    return bits;
}

// Chunks of the whole problem at most: a gene wastes less than one.
uint64_t chunkBound(uint64_t entryCount, uint32_t geneCount) { return entryCount / kChunk + geneCount; }

std::atomic<uint32_t> maxBlocks{0};

// Waves that stride over `items`: blocks of 4, at most 65536 blocks (or what setGeneInformationMaxBlocks asked for).
uint32_t waveGridFor(uint64_t items)
{
    const uint64_t blocks = (items + 3u) / 4u;
    const uint32_t asked = maxBlocks.load();
    const uint32_t most = asked ? asked : 65536u;
    return uint32_t(blocks > most ? most : (blocks ? blocks : 1u));
}

struct Layout {
    size_t words, keysA, keysB, valuesA, valuesB, offsets, chunkCounts, chunkStarts, table, partials, sums, inverseSums, sortTemp, scanTemp, total;
    size_t sortTempBytes, scanTempBytes;
};

hipError_t layoutOf(uint64_t entryCount, uint32_t geneCount, Layout& l)
{
    ArenaPlan plan;
    const size_t perGene = (size_t(geneCount) + 1u) * sizeof(uint64_t);
    l.words = plan.take(256);
    l.keysA = plan.takeFor<uint32_t>(entryCount);
    l.keysB = plan.takeFor<uint32_t>(entryCount);
    l.valuesA = plan.takeFor<float>(entryCount);
    l.valuesB = plan.takeFor<float>(entryCount);
    l.offsets = plan.take(perGene);
    l.chunkCounts = plan.take(perGene);
    l.chunkStarts = plan.take(perGene);
    l.table = plan.takeFor<ChunkRef>(chunkBound(entryCount, geneCount));
    l.partials = plan.takeFor<double>(chunkBound(entryCount, geneCount));
    l.sums = plan.take(perGene);
    l.inverseSums = plan.take(perGene);
    l.sortTempBytes = 0;
    if (entryCount && geneBitsOf(geneCount)) {
        EM2_TRY(sortPairsU32F32BufferBytes(size_t(entryCount), 0u, geneBitsOf(geneCount), l.sortTempBytes));
    }
    l.scanTempBytes = 0;
    EM2_TRY(exclusiveScanU64Bytes(size_t(geneCount) + 1u, l.scanTempBytes));
    l.sortTemp = plan.take(l.sortTempBytes);
    l.scanTemp = plan.take(l.scanTempBytes);
    l.total = plan.bytes;
    return hipSuccess;
}

}  // namespace

void setGeneInformationMaxBlocks(uint32_t blocks) { maxBlocks.store(blocks); }

size_t geneInformationWorkspaceBytes(uint64_t entryCount, uint32_t geneCount)
{
    Layout l;
    return layoutOf(entryCount, geneCount, l) == hipSuccess ? l.total : 0;
}

hipError_t launchCellNormInverses(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, int method,
                                  double* normInverse, hipStream_t stream)
{
    if (cellCount == 0) return hipSuccess;
    cellNormInversesKernel<<<dim3(gridFor(cellCount)), dim3(256), 0, stream>>>(toc, data, cellCount, geneCount, method, normInverse);
    return hipGetLastError();
}

hipError_t runGeneInformation(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                              const double* d_normInverse, double logN, double log2, float* d_informationContent,
                              double* d_informationContentDouble, uint32_t* d_expressingCellCount, void* workspace, size_t workspaceBytes,
                              uint32_t* inputError, hipStream_t stream)
{
    *inputError = 0;
    Layout l;
    EM2_TRY(layoutOf(entryCount, geneCount, l));
    if (workspaceBytes < l.total) return hipErrorInvalidValue;
    StageTimer timer("geneInformationContent");
    char* base = static_cast<char*>(workspace);
    uint32_t* words = arenaAt<uint32_t>(base, l.words);
    uint64_t* offsets = arenaAt<uint64_t>(base, l.offsets);
    uint64_t* chunkCounts = arenaAt<uint64_t>(base, l.chunkCounts);
    uint64_t* chunkStarts = arenaAt<uint64_t>(base, l.chunkStarts);
    ChunkRef* table = arenaAt<ChunkRef>(base, l.table);
    double* partials = arenaAt<double>(base, l.partials);
    double* sums = arenaAt<double>(base, l.sums);
    double* inverseSums = arenaAt<double>(base, l.inverseSums);
    DoubleBuffer<uint32_t> keys{arenaAt<uint32_t>(base, l.keysA), arenaAt<uint32_t>(base, l.keysB)};
    DoubleBuffer<float> values{arenaAt<float>(base, l.valuesA), arenaAt<float>(base, l.valuesB)};

    EM2_TRY(hipMemsetAsync(words, 0, 256, stream));
    entriesKernel<<<dim3(waveGridFor(cellCount)), dim3(256), 0, stream>>>(d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse,
                                                                          keys.current(), values.current(), words);
    EM2_TRY(hipGetLastError());
    // the gene ids are the sort's keys and the segments' bounds: nothing goes on before they are known to be good
    EM2_TRY(hipMemcpyAsync(inputError, words, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    if (*inputError) return hipSuccess;
    EM2_TRY(timer.stage("entries", stream));

    // one gene (no key bits): the stream is in cell order already
    if (entryCount && geneBitsOf(geneCount)) {
        EM2_TRY(sortPairs(base + l.sortTemp, l.sortTempBytes, keys, values, size_t(entryCount), 0u, geneBitsOf(geneCount), stream));
    }
    EM2_TRY(timer.stage("sort", stream));

    geneSegmentsKernel<<<dim3(gridFor(uint64_t(geneCount) + 1u)), dim3(256), 0, stream>>>(keys.current(), entryCount, geneCount, offsets,
                                                                                         chunkCounts, d_expressingCellCount);
    EM2_TRY(hipGetLastError());
    EM2_TRY(exclusiveScan(base + l.scanTemp, l.scanTempBytes, chunkCounts, chunkStarts, size_t(geneCount) + 1u, stream));
    const uint64_t bound = chunkBound(entryCount, geneCount);
    chunkTableKernel<<<dim3(gridFor(bound)), dim3(256), 0, stream>>>(chunkStarts, geneCount, table);
    EM2_TRY(hipGetLastError());
    EM2_TRY(timer.stage("segments and chunk table", stream));

    chunkReduceKernel<0><<<dim3(waveGridFor(bound)), dim3(256), 0, stream>>>(values.current(), offsets, chunkStarts, geneCount, table, nullptr,
                                                                            partials);
    geneSumsKernel<<<dim3(gridFor(geneCount)), dim3(256), 0, stream>>>(partials, chunkStarts, geneCount, words, sums, inverseSums);
    EM2_TRY(hipGetLastError());
    EM2_TRY(timer.stage("pass 1 (sums)", stream));
    chunkReduceKernel<1><<<dim3(waveGridFor(bound)), dim3(256), 0, stream>>>(values.current(), offsets, chunkStarts, geneCount, table,
                                                                            inverseSums, partials);
    geneFinishKernel<<<dim3(gridFor(geneCount)), dim3(256), 0, stream>>>(partials, chunkStarts, geneCount, logN, log2, d_informationContent,
                                                                         d_informationContentDouble);
    EM2_TRY(hipGetLastError());
    EM2_TRY(hipStreamSynchronize(stream));
    EM2_TRY(timer.stage("pass 2 (terms) and finish", stream));
    return hipSuccess;
}

}  // namespace em2


// ---- the C entry points (include/em2_lsh.h) ----

using namespace em2::entry;
using em2::DeviceBuffer;

extern "C" {

static const char* geneInformationErrorText(uint32_t inputError)
{
    return (inputError & 4u) ? "toc does not start at 0, does not end at entryCount or is not ascending" : em2::inputErrorText(inputError);
}

// Cell::norm1Inverse / norm2Inverse as ExpressionMatrix::addCell defines them (src/ExpressionMatrix.cpp:241-263), on the host:
// walkCell's arithmetic (em2_expression.h) and its checks.
int em2_cell_norm_inverses(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, double* norm1Inverse,
                           double* norm2Inverse)
{
    const char* who = "em2_cell_norm_inverses";
    if (cellCount == 0) return EM2_OK;
    if (!toc || !norm1Inverse || !norm2Inverse) return failNull(who);
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    uint32_t bad = 0;
    for (uint32_t cell = 0; cell < cellCount; ++cell) {
        double sum1 = 0., sum2 = 0.;
        for (uint64_t p = toc[cell]; p < toc[cell + 1]; ++p) {
            if (data[p].gene >= geneCount) bad |= 1u;
            if (p != toc[cell] && data[p].gene <= data[p - 1].gene) bad |= 2u;
            const float value = data[p].count;
            sum1 += double(value);
            sum2 += double(value * value);                  // a float product (:258)
        }
        norm1Inverse[cell] = 1. / sum1;
        norm2Inverse[cell] = 1. / std::sqrt(sum2);
    }
    if (bad) return failArgument(who, em2::inputErrorText(bad));
    return EM2_OK;
}

void em2_set_gene_information_max_blocks(uint32_t blocks) { em2::setGeneInformationMaxBlocks(blocks); }

size_t em2_dev_gene_information_content_workspace(uint32_t cellCount, uint32_t geneCount, uint64_t entryCount)
{
    (void)cellCount;
    return em2::geneInformationWorkspaceBytes(entryCount, geneCount);
}

// The device call under the name of the entry point that makes it.
static int devGeneInformation(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                              uint64_t entryCount, const double* d_normInverse, float* d_informationContent,
                              double* d_informationContentDouble, uint32_t* d_expressingCellCount, void* d_workspace,
                              size_t workspaceBytes, void* stream)
{
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (!d_toc || !d_informationContent || !d_workspace || (!d_data && entryCount)) return failNull(who);
    if (workspaceBytes < em2::geneInformationWorkspaceBytes(entryCount, geneCount)) return failArgument(who, "workspace too small");
    uint32_t inputError = 0;
    // :2004 and :2015 with the host's log, so that a gene without a positive entry gets the reference's float exactly
    EM2_HIP(em2::runGeneInformation(d_toc, reinterpret_cast<const em2::CountIn*>(d_data), cellCount, geneCount, entryCount, d_normInverse,
                                    std::log(double(cellCount)), std::log(2.), d_informationContent, d_informationContentDouble,
                                    d_expressingCellCount, d_workspace, workspaceBytes, &inputError, static_cast<hipStream_t>(stream)));
    if (inputError) return failArgument(who, geneInformationErrorText(inputError));
    return EM2_OK;
}

int em2_dev_gene_information_content(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                                     uint64_t entryCount, const double* d_normInverse, float* d_informationContent,
                                     double* d_informationContentDouble, uint32_t* d_expressingCellCount, void* d_workspace,
                                     size_t workspaceBytes, void* stream)
{
    return devGeneInformation("em2_dev_gene_information_content", d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse,
                              d_informationContent, d_informationContentDouble, d_expressingCellCount, d_workspace, workspaceBytes, stream);
}

// The device call on a CSR that is on the device already; the results to the host.
static int geneInformationToHost(const char* who, const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                                 uint64_t entryCount, const double* d_normInverse, float* informationContent,
                                 double* informationContentDouble, uint32_t* expressingCellCount)
{
    DeviceBuffer dFloat, dDouble, dExpressing, dWorkspace;
    const size_t workspaceBytes = em2::geneInformationWorkspaceBytes(entryCount, geneCount);
    EM2_HIP(dFloat.allocateFor<float>(geneCount));
    if (informationContentDouble) EM2_HIP(dDouble.allocateFor<double>(geneCount));
    if (expressingCellCount) EM2_HIP(dExpressing.allocateFor<uint32_t>(geneCount));
    EM2_HIP(dWorkspace.allocate(workspaceBytes));
    const int rc = devGeneInformation(who, d_toc, d_data, cellCount, geneCount, entryCount, d_normInverse, dFloat.as<float>(),
                                      dDouble.as<double>(), dExpressing.as<uint32_t>(), dWorkspace.p, workspaceBytes, nullptr);
    if (rc != EM2_OK) return rc;
    if (informationContent) EM2_HIP(dFloat.download(informationContent, geneCount));
    if (informationContentDouble) EM2_HIP(dDouble.download(informationContentDouble, geneCount));
    if (expressingCellCount) EM2_HIP(dExpressing.download(expressingCellCount, geneCount));
    return EM2_OK;
}

int em2_gene_information_content(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                 const double* normInverse, float* informationContent, double* informationContentDouble,
                                 uint32_t* expressingCellCount)
{
    const char* who = "em2_gene_information_content";
    if (geneCount == 0) return failArgument(who, "geneCount must be positive");
    if (cellCount == 0) return failArgument(who, "cellCount must be positive");
    if (!toc || !informationContent) return failNull(who);
    em2::UploadedCsr csr;
    if (const char* error = csr.check(toc, reinterpret_cast<const em2::CountIn*>(data), cellCount)) return failArgument(who, error);
    if (!haveDevice()) return failNoDevice(who);
    EM2_HIP(csr.upload());                     // (the device checks the gene ids before any kernel indexes with them)
    DeviceBuffer dNorm;
    if (normInverse) EM2_HIP(dNorm.upload(normInverse, cellCount));
    return geneInformationToHost(who, csr.toc.as<uint64_t>(), csr.data.as<em2_count>(), cellCount, geneCount, csr.nnz,
                                 normInverse ? dNorm.as<double>() : nullptr, informationContent, informationContentDouble, expressingCellCount);
}

// The matrix-level call (em2_host.cpp): the rows of the cell set go to the device with their global gene ids; the cells' norm
// inverses are taken over those WHOLE rows there (or come from the Cells file: normInverseOfRows, one per row), the gene set
// is applied by the device subset, and the rest is em2_dev_gene_information_content.  rowToc from 0.  Internal to the library.
int em2_internal_gene_information(const uint64_t* rowToc, const em2_count* rowData, uint32_t cellCount, const uint32_t* geneLocalIds,
                                  uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod, const double* normInverseOfRows,
                                  float* informationContent, uint32_t* expressingCellCount)
{
    const char* who = "em2_matrix_gene_information_content";
    if (normalizationMethod < 0 || normalizationMethod > 2) return failArgument(who, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (!haveDevice()) return failNoDevice(who);
    em2::UploadedCsr rows;
    if (const char* error = rows.check(rowToc, reinterpret_cast<const em2::CountIn*>(rowData), cellCount)) return failArgument(who, error);
    EM2_HIP(rows.upload());
    DeviceBuffer dNorm, dLocalIds, dToc, dData, dSubsetWorkspace;
    if (normalizationMethod != 0) {
        if (normInverseOfRows) {
            EM2_HIP(dNorm.upload(normInverseOfRows, cellCount));
        } else {
            EM2_HIP(dNorm.allocateFor<double>(cellCount));
            // (a global gene id is checked by nothing here: the subset below drops what the gene set does not know)
            EM2_HIP(em2::launchCellNormInverses(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), cellCount, 0xffffffffu,
                                                normalizationMethod, dNorm.as<double>(), nullptr));
        }
    }
    const size_t subsetBytes = em2::subsetWorkspaceBytes(cellCount);
    EM2_HIP(dLocalIds.upload(geneLocalIds, globalGeneCount));
    EM2_HIP(dToc.allocateFor<uint64_t>(size_t(cellCount) + 1));
    EM2_HIP(dSubsetWorkspace.allocate(subsetBytes));
    EM2_HIP(em2::launchSubsetCount(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), nullptr, cellCount, dLocalIds.as<uint32_t>(),
                                   globalGeneCount, dToc.as<uint64_t>(), dSubsetWorkspace.p, subsetBytes, nullptr));
    uint64_t entryCount = 0;
    EM2_HIP(hipMemcpy(&entryCount, dToc.as<uint64_t>() + cellCount, sizeof(uint64_t), hipMemcpyDeviceToHost));
    EM2_HIP(dData.allocateFor<em2_count>(entryCount));
    EM2_HIP(em2::launchSubsetFill(rows.toc.as<uint64_t>(), rows.data.as<em2::CountIn>(), nullptr, cellCount, dLocalIds.as<uint32_t>(),
                                  globalGeneCount, dToc.as<uint64_t>(), dData.as<em2::CountIn>(), nullptr));
    return geneInformationToHost(who, dToc.as<uint64_t>(), dData.as<em2_count>(), cellCount, geneCount, entryCount,
                                 normalizationMethod != 0 ? dNorm.as<double>() : nullptr, informationContent, nullptr, expressingCellCount);
}

}  // extern "C"
