// em2_ingest.hip -- the device pass of the bulk add (ExpressionMatrix::addCell's storing part, src/ExpressionMatrix.cpp:241-277,
// for every barcode of a sparse matrix at once): em2_dev_ingest_count, em2_dev_ingest_fill and the host driver's chunk call.
//
// One kernel body serves both passes and all row lengths.  A row is read once: its entries that are not zero go, in input
// order, with their gene ids from the map, into a buffer; the sums are taken from the buffer in that order; the buffer is
// sorted by gene id with a bitonic network of this file (every comparator puts the smaller gene at the lower index, so a
// length that is no power of two needs no padding: the missing elements would be +infinity at the top and never move);
// neighbours with equal genes are the duplicates.  The count pass ends there (kept entries, status, smallest duplicated gene);
// the fill pass writes the buffer to the cell's place in the output and the 56-byte Cell record.
//
//   rows of at most kWaveRowLimit entries        a wave (a block of 64 threads), 4 KiB of LDS
//   rows up to the LDS row limit                 a workgroup of 256 threads, 8 bytes of LDS per entry (64 KiB by default)
//   longer rows                                  a workgroup sorting in global memory: in the cell's output place (fill) or
//                                                in scratch as long as the input (count)
//
// sum1 and sum2 are the reference's sequential double sums bit for bit: one lane adds in input order, unless every kept
// value is a finite integer and kept * largest^2 <= 2^52 -- then every float square is an integer, every partial sum in any
// order is an integer below 2^53, nothing is ever rounded, and the lanes add in parallel.  The square is a float product
// (__fmul_rn: never contracted), sqrt and the divisions are __dsqrt_rn and __ddiv_rn.
#include "em2_ingest.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_wave.h"

#include <cstring>

#include <atomic>
#include <string>

using namespace em2::entry;

namespace em2 {

namespace {

struct Entry {
    uint32_t gene;
    float value;
};
static_assert(sizeof(Entry) == sizeof(em2_count), "an entry is a std::pair<GeneId, float>");

constexpr uint32_t kWaveRowLimit = 512;
constexpr uint32_t kDefaultLdsRowLimit = 8192;
constexpr uint32_t kMaxLdsRowLimit = 16384;                // 128 KiB of the 160 KiB a workgroup may declare
constexpr uint32_t kNoGene = 0xffffffffu;

std::atomic<uint32_t> ldsRowLimitSetting{0};

struct RowResult {
    uint32_t kept, status, duplicateGene;
    double sum1, sum2;                                      // valid in thread 0
};

// sU32: [0, 4) the waves' kept counts, [4, 8) their largest values, [8] the smallest duplicated gene.  sF64: [0, 8).
template <uint32_t THREADS>
__device__ __forceinline__ RowResult ingestRow(Entry* buf, uint32_t capacity, const uint32_t* __restrict__ indices,
                                               const float* __restrict__ values, uint32_t length,
                                               const uint32_t* __restrict__ geneIdOfIndex, uint32_t indexCount, uint32_t* sU32, double* sF64)
{
    constexpr uint32_t WAVES = THREADS / 64u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    if (tid == 0) sU32[8] = kNoGene;

    // the entries that are not zero, in input order (:251-259)
    uint32_t kept = 0;
    bool negative = false, badIndex = false, integral = true;
    float largest = 0.f;
    for (uint32_t offset = 0; offset < length; offset += THREADS) {
        const uint32_t i = offset + tid;
        float value = 0.f;
        uint32_t gene = 0;
        bool keep = false;
        if (i < length) {
            value = values[i];
            negative = negative || value < 0.f;
            keep = value != 0.f;                                              // NaN is kept
            if (keep) {
                const uint32_t index = indices[i];
                if (index < indexCount) gene = geneIdOfIndex[index];
                else badIndex = true;
                integral = integral && fabsf(value) < __builtin_inff() && value == truncf(value);
                largest = fmaxf(largest, value);
            }
        }
        const uint64_t mask = __ballot(keep);
        uint32_t at = kept + lanesBelow(mask), total = uint32_t(__popcll(mask));
        if (WAVES > 1u) {
            if (lane == 0) sU32[wave] = total;
            __syncthreads();
            total = 0;
            for (uint32_t w = 0; w < WAVES; w++) {
                if (w < wave) at += sU32[w];
                total += sU32[w];
            }
            __syncthreads();
        }
        if (keep && at < capacity) {
            Entry e;
            e.gene = gene;
            e.value = value;
            buf[at] = e;
        }
        kept += total;
    }
    negative = __syncthreads_or(negative ? 1 : 0) != 0;
    badIndex = __syncthreads_or(badIndex ? 1 : 0) != 0;
    integral = __syncthreads_and(integral ? 1 : 0) != 0;
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) largest = fmaxf(largest, __shfl_xor(largest, step, 64));
    if (WAVES > 1u) {
        if (lane == 0) sU32[4u + wave] = __float_as_uint(largest);
        __syncthreads();
        for (uint32_t w = 0; w < WAVES; w++) largest = fmaxf(largest, __uint_as_float(sU32[4u + w]));
    }
    RowResult r{kept, 0u, kNoGene, 0., 0.};
    if (kept > capacity) {                                                    // (the caller's toc is not this row's: nothing is sorted)
        r.status = 4u;
        __syncthreads();
        return r;
    }

    // the sums (:257-258)
    const bool exact = integral && !negative && double(largest) * double(largest) * double(kept) <= 0x1p52;
    if (exact) {
        double sum1 = 0., sum2 = 0.;
        for (uint32_t i = tid; i < kept; i += THREADS) {
            const float value = buf[i].value;
            sum1 += double(value);
            sum2 += double(__fmul_rn(value, value));
        }
        sum1 = waveSum(sum1);
        sum2 = waveSum(sum2);
        if (WAVES > 1u) {
            if (lane == 0) {
                sF64[wave] = sum1;
                sF64[WAVES + wave] = sum2;
            }
            __syncthreads();
            sum1 = sum2 = 0.;
            for (uint32_t w = 0; w < WAVES; w++) {
                sum1 += sF64[w];
                sum2 += sF64[WAVES + w];
            }
        }
        r.sum1 = sum1;
        r.sum2 = sum2;
    } else if (tid == 0) {
        double sum1 = 0., sum2 = 0.;
        for (uint32_t i = 0; i < kept; i++) {
            const float value = buf[i].value;
            sum1 += double(value);
            sum2 += double(__fmul_rn(value, value));
        }
        r.sum1 = sum1;
        r.sum2 = sum2;
    }
    __syncthreads();

    // ascending by gene id (:266-267)
    for (uint64_t k = 2; (k >> 1) < kept; k <<= 1) {
        for (uint64_t j = k >> 1; j > 0; j >>= 1) {
            const uint32_t flip = uint32_t(j == (k >> 1) ? k - 1u : j);     // the first step of a merge mirrors, the others halve
            for (uint32_t i = tid; i < kept; i += THREADS) {
                const uint32_t partner = i ^ flip;
                if (partner > i && partner < kept) {
                    const Entry a = buf[i], b = buf[partner];
                    if (b.gene < a.gene) {
                        buf[i] = b;
                        buf[partner] = a;
                    }
                }
            }
            __syncthreads();
        }
    }

    // distinct genes (:272-277): the smallest gene that two kept entries share
    for (uint32_t i = tid + 1u; i < kept; i += THREADS) {
        const uint32_t gene = buf[i].gene;
        if (buf[i - 1u].gene == gene) atomicMin(&sU32[8], gene);
    }
    __syncthreads();
    r.duplicateGene = sU32[8];
    r.status = badIndex ? uint32_t(host::kIngestBadIndex)
                        : (negative ? uint32_t(host::kIngestNegative) : (r.duplicateGene != kNoGene ? uint32_t(host::kIngestDuplicate) : 0u));
    if (r.status != uint32_t(host::kIngestDuplicate)) r.duplicateGene = kNoGene;
    __syncthreads();
    return r;
}

struct IngestArguments {
    const uint64_t* indptr;
    const uint32_t* indices;
    const float* values;
    const uint8_t* skip;
    uint32_t cellCount;
    const uint32_t* geneIdOfIndex;
    uint32_t indexCount;
    uint32_t waveLimit, ldsLimit;
    // the count pass
    uint32_t* keptCount;
    uint32_t* status;
    uint32_t* duplicateGene;
    Entry* scratch;                                         // [indptr[cellCount]], rows above the LDS limit only
    // the fill pass
    const uint64_t* outToc;
    Entry* outData;
    double* outCells;                                       // 7 per cell
    uint32_t* error;                                        // a row whose kept entries are not what outToc says
    // the rows of the workgroup kernels
    const uint32_t* list;
    const uint32_t* listCount;
};

// MODE 0: a wave per row, every row that is short enough; 1: a workgroup per listed row, LDS; 2: the same in global memory.
template <uint32_t THREADS, int MODE, bool FILL>
__global__ __launch_bounds__(THREADS) void ingestKernel(const IngestArguments a)
{
    __shared__ uint32_t sU32[16];
    __shared__ double sF64[8];
    __shared__ Entry waveBuffer[MODE == 0 ? kWaveRowLimit : 1u];
    extern __shared__ __align__(8) unsigned char dynamicLds[];
    const uint32_t rowCount = MODE == 0 ? a.cellCount : *a.listCount;
    for (uint32_t n = blockIdx.x; n < rowCount; n += gridDim.x) {
        const uint32_t row = MODE == 0 ? n : a.list[n];
        const uint64_t begin = a.indptr[row];
        const uint32_t length = uint32_t(a.indptr[row + 1u] - begin);
        const bool skipped = a.skip && a.skip[row];
        if (MODE == 0) {
            if (skipped) {                                                    // neither named nor checked
                if (!FILL && threadIdx.x == 0) {
                    a.keptCount[row] = 0u;
                    a.status[row] = 0u;
                    a.duplicateGene[row] = kNoGene;
                }
                continue;
            }
            if (length > a.waveLimit) continue;
        }
        const uint64_t outBegin = FILL ? a.outToc[row] : 0u;
        const uint64_t outLength = FILL ? a.outToc[row + 1u] - outBegin : 0u;
        Entry* buf;
        uint32_t capacity = length;
        if (MODE == 0) {
            buf = waveBuffer;
        } else if (MODE == 1) {
            buf = reinterpret_cast<Entry*>(dynamicLds);
        } else if (FILL) {
            buf = a.outData + outBegin;
            capacity = outLength < length ? uint32_t(outLength) : length;
        } else {
            buf = a.scratch + begin;
        }
        const RowResult r = ingestRow<THREADS>(buf, capacity, a.indices + begin, a.values + begin, length, a.geneIdOfIndex, a.indexCount,
                                               sU32, sF64);
        if (!FILL) {
            if (threadIdx.x == 0) {
                a.keptCount[row] = r.kept;
                a.status[row] = r.status;
                a.duplicateGene[row] = r.duplicateGene;
            }
        } else if (r.kept != outLength || r.status == 4u) {
            if (threadIdx.x == 0) atomicOr(a.error, 1u);
        } else {
            if (MODE != 2) {
                Entry* out = a.outData + outBegin;
                for (uint32_t i = threadIdx.x; i < r.kept; i += THREADS) out[i] = buf[i];
            }
            if (threadIdx.x == 0) {                                           // :261-263; the last two doubles are written as 0
                double* cell = a.outCells + size_t(row) * 7u;
                const double norm2 = __dsqrt_rn(r.sum2);
                cell[0] = r.sum1;
                cell[1] = r.sum2;
                cell[2] = norm2;
                cell[3] = __ddiv_rn(1., r.sum1);
                cell[4] = __ddiv_rn(1., norm2);
                cell[5] = 0.;
                cell[6] = 0.;
            }
        }
        __syncthreads();                                                      // (the buffer is the next row's)
    }
}

// lists[0, cellCount): the rows of the LDS workgroup kernel; lists[cellCount, 2 cellCount): those of the global-memory one.
__global__ void ingestClassifyKernel(const uint64_t* __restrict__ indptr, const uint8_t* __restrict__ skip, uint32_t cellCount,
                                     uint32_t waveLimit, uint32_t ldsLimit, uint32_t* lists, uint32_t* counters)
{
    for (uint64_t row = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; row < cellCount; row += uint64_t(gridDim.x) * blockDim.x) {
        if (skip && skip[row]) continue;
        const uint64_t length = indptr[row + 1u] - indptr[row];
        if (length <= waveLimit) continue;
        if (length <= ldsLimit) lists[atomicAdd(&counters[0], 1u)] = uint32_t(row);
        else lists[size_t(cellCount) + atomicAdd(&counters[1], 1u)] = uint32_t(row);
    }
}

__global__ void ingestLastOffsetKernel(const uint32_t* keptCount, uint64_t* outToc, uint32_t cellCount)
{
    outToc[cellCount] = outToc[cellCount - 1u] + keptCount[cellCount - 1u];
}

template <bool FILL>
hipError_t runIngest(IngestArguments a, uint64_t* outTocOfCount, uint32_t* error, hipStream_t stream)
{
    *error = 0;
    if (a.cellCount == 0) return hipSuccess;
    const uint32_t setting = ldsRowLimitSetting.load();
    a.ldsLimit = setting ? setting : kDefaultLdsRowLimit;
    a.waveLimit = a.ldsLimit < kWaveRowLimit ? a.ldsLimit : kWaveRowLimit;
    DeviceBuffer lists, counters, scratch, scanTemp;
    EM2_TRY(lists.allocate(size_t(a.cellCount) * 2u * sizeof(uint32_t)));
    EM2_TRY(counters.allocate(3u * sizeof(uint32_t)));
    EM2_TRY(hipMemsetAsync(counters.p, 0, 3u * sizeof(uint32_t), stream));
    a.error = counters.as<uint32_t>() + 2;
    ingestClassifyKernel<<<dim3(gridFor(a.cellCount)), dim3(256), 0, stream>>>(a.indptr, a.skip, a.cellCount, a.waveLimit, a.ldsLimit,
                                                                               lists.as<uint32_t>(), counters.as<uint32_t>());
    EM2_TRY(hipGetLastError());
    uint32_t listCounts[2] = {0, 0};
    EM2_TRY(hipMemcpyAsync(listCounts, counters.p, sizeof(listCounts), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));

    const uint32_t waveBlocks = a.cellCount < (1u << 20) ? a.cellCount : (1u << 20);
    ingestKernel<64, 0, FILL><<<dim3(waveBlocks), dim3(64), 0, stream>>>(a);
    EM2_TRY(hipGetLastError());
    if (listCounts[0]) {
        a.list = lists.as<uint32_t>();
        a.listCount = counters.as<uint32_t>();
        const int ldsBytes = int(a.ldsLimit * sizeof(Entry));
        EM2_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(ingestKernel<256, 1, FILL>), hipFuncAttributeMaxDynamicSharedMemorySize, ldsBytes));
        ingestKernel<256, 1, FILL><<<dim3(listCounts[0] < 4096u ? listCounts[0] : 4096u), dim3(256), size_t(ldsBytes), stream>>>(a);
        EM2_TRY(hipGetLastError());
    }
    if (listCounts[1]) {
        a.list = lists.as<uint32_t>() + a.cellCount;
        a.listCount = counters.as<uint32_t>() + 1;
        if (!FILL) {
            uint64_t entryCount = 0;
            EM2_TRY(hipMemcpyAsync(&entryCount, a.indptr + a.cellCount, sizeof(entryCount), hipMemcpyDeviceToHost, stream));
            EM2_TRY(hipStreamSynchronize(stream));
            EM2_TRY(scratch.allocate(size_t(entryCount) * sizeof(Entry)));
            a.scratch = scratch.as<Entry>();
        }
        ingestKernel<256, 2, FILL><<<dim3(listCounts[1] < 1024u ? listCounts[1] : 1024u), dim3(256), 0, stream>>>(a);
        EM2_TRY(hipGetLastError());
    }
    if (!FILL) {                                                              // the cells' places in the output
        size_t tempBytes = 0;
        EM2_TRY(exclusiveScanU32ToU64Bytes(size_t(a.cellCount), tempBytes));
        EM2_TRY(scanTemp.allocate(tempBytes));
        EM2_TRY(exclusiveScan(scanTemp.p, tempBytes, a.keptCount, outTocOfCount, size_t(a.cellCount), stream));
        ingestLastOffsetKernel<<<dim3(1), dim3(1), 0, stream>>>(a.keptCount, outTocOfCount, a.cellCount);
        EM2_TRY(hipGetLastError());
    } else {
        EM2_TRY(hipMemcpyAsync(error, a.error, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    return hipStreamSynchronize(stream);                                      // (the lists and the scratch end with this call)
}

int devIngestCount(const char* who, const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                   uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, uint32_t* d_keptCount, uint32_t* d_status,
                   uint32_t* d_duplicateGene, uint64_t* d_outToc, void* stream)
{
    if (!d_indptr || !d_outToc || (cellCount && (!d_keptCount || !d_status || !d_duplicateGene))) return failNull(who);
    if (!haveDevice()) return failNoDevice(who);
    if (cellCount == 0) {
        EM2_HIP_FOR(who, hipMemsetAsync(d_outToc, 0, sizeof(uint64_t), static_cast<hipStream_t>(stream)));
        return EM2_OK;
    }
    IngestArguments a{};
    a.indptr = d_indptr;
    a.indices = d_indices;
    a.values = d_values;
    a.skip = d_skip;
    a.cellCount = cellCount;
    a.geneIdOfIndex = d_geneIdOfIndex;
    a.indexCount = indexCount;
    a.keptCount = d_keptCount;
    a.status = d_status;
    a.duplicateGene = d_duplicateGene;
    uint32_t error = 0;
    EM2_HIP_FOR(who, runIngest<false>(a, d_outToc, &error, static_cast<hipStream_t>(stream)));
    return EM2_OK;
}

int devIngestFill(const char* who, const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                  uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, const uint64_t* d_outToc, em2_count* d_outData,
                  void* d_outCells, void* stream)
{
    if (cellCount == 0) return EM2_OK;
    if (!d_indptr || !d_outToc || !d_outData || !d_outCells) return failNull(who);
    if (reinterpret_cast<uintptr_t>(d_outCells) % sizeof(double)) return failArgument(who, "d_outCells is not aligned to a double");
    if (!haveDevice()) return failNoDevice(who);
    IngestArguments a{};
    a.indptr = d_indptr;
    a.indices = d_indices;
    a.values = d_values;
    a.skip = d_skip;
    a.cellCount = cellCount;
    a.geneIdOfIndex = d_geneIdOfIndex;
    a.indexCount = indexCount;
    a.outToc = d_outToc;
    a.outData = reinterpret_cast<Entry*>(d_outData);
    a.outCells = static_cast<double*>(d_outCells);
    uint32_t error = 0;
    EM2_HIP_FOR(who, runIngest<true>(a, nullptr, &error, static_cast<hipStream_t>(stream)));
    if (error) return failArgument(who, "d_outToc is not what the count pass gives for these rows");
    return EM2_OK;
}

}  // namespace

namespace host {

int ingestChunkOnDevice(const uint64_t* indptr, const uint32_t* indices, const float* values, const uint8_t* skip, uint32_t cellCount,
                        const uint32_t* geneIdOfIndex, uint32_t indexCount, std::vector<uint32_t>& keptCount,
                        std::vector<uint32_t>& status, std::vector<uint32_t>& duplicateGene, std::vector<uint64_t>& toc,
                        std::vector<em2_count>& data, std::vector<CellRecord>& cells, bool* failed)
{
    const char* who = "em2_matrix_add_cells_csr";
    *failed = false;
    if (!haveDevice()) return failNoDevice(who);
    const uint64_t entryCount = indptr[cellCount];
    DeviceBuffer dIndptr, dIndices, dValues, dSkip, dGenes, dKept, dStatus, dDuplicate, dToc, dData, dCells;
    EM2_HIP_FOR(who, dIndptr.upload(indptr, size_t(cellCount) + 1u));
    EM2_HIP_FOR(who, dIndices.upload(indices, size_t(entryCount)));
    EM2_HIP_FOR(who, dValues.upload(values, size_t(entryCount)));
    EM2_HIP_FOR(who, dSkip.upload(skip, cellCount));
    EM2_HIP_FOR(who, dGenes.upload(geneIdOfIndex, indexCount));
    EM2_HIP_FOR(who, dKept.allocateFor<uint32_t>(cellCount));
    EM2_HIP_FOR(who, dStatus.allocateFor<uint32_t>(cellCount));
    EM2_HIP_FOR(who, dDuplicate.allocateFor<uint32_t>(cellCount));
    EM2_HIP_FOR(who, dToc.allocateFor<uint64_t>(size_t(cellCount) + 1u));
    int rc = devIngestCount(who, dIndptr.as<uint64_t>(), dIndices.as<uint32_t>(), dValues.as<float>(), dSkip.as<uint8_t>(), cellCount,
                            dGenes.as<uint32_t>(), indexCount, dKept.as<uint32_t>(), dStatus.as<uint32_t>(), dDuplicate.as<uint32_t>(),
                            dToc.as<uint64_t>(), nullptr);
    if (rc != EM2_OK) return rc;
    keptCount.resize(cellCount);
    status.resize(cellCount);
    duplicateGene.resize(cellCount);
    toc.resize(size_t(cellCount) + 1u);
    EM2_HIP_FOR(who, dKept.download(keptCount.data(), cellCount));
    EM2_HIP_FOR(who, dStatus.download(status.data(), cellCount));
    EM2_HIP_FOR(who, dDuplicate.download(duplicateGene.data(), cellCount));
    EM2_HIP_FOR(who, dToc.download(toc.data(), size_t(cellCount) + 1u));
    for (uint32_t i = 0; i < cellCount; i++) {
        if (status[i] != 0u) *failed = true;
    }
    data.clear();
    cells.assign(cellCount, CellRecord());
    if (*failed) return EM2_OK;
    const uint64_t outCount = toc[cellCount];
    EM2_HIP_FOR(who, dData.allocateFor<em2_count>(size_t(outCount)));
    EM2_HIP_FOR(who, dCells.allocateFor<CellRecord>(cellCount));
    EM2_HIP_FOR(who, hipMemset(dCells.p, 0, size_t(cellCount) * sizeof(CellRecord)));
    rc = devIngestFill(who, dIndptr.as<uint64_t>(), dIndices.as<uint32_t>(), dValues.as<float>(), dSkip.as<uint8_t>(), cellCount,
                       dGenes.as<uint32_t>(), indexCount, dToc.as<uint64_t>(), dData.as<em2_count>(), dCells.p, nullptr);
    if (rc != EM2_OK) return rc;
    data.resize(size_t(outCount));
    EM2_HIP_FOR(who, dData.download(data.data(), size_t(outCount)));
    EM2_HIP_FOR(who, dCells.download(cells.data(), cellCount));
    return EM2_OK;
}

}  // namespace host
}  // namespace em2

extern "C" {

int em2_dev_ingest_count(const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                         uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, uint32_t* d_keptCount,
                         uint32_t* d_status, uint32_t* d_duplicateGene, uint64_t* d_outToc, void* stream)
{
    return em2::devIngestCount("em2_dev_ingest_count", d_indptr, d_indices, d_values, d_skip, cellCount, d_geneIdOfIndex, indexCount,
                               d_keptCount, d_status, d_duplicateGene, d_outToc, stream);
}

int em2_dev_ingest_fill(const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                        uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, const uint64_t* d_outToc,
                        em2_count* d_outData, void* d_outCells, void* stream)
{
    return em2::devIngestFill("em2_dev_ingest_fill", d_indptr, d_indices, d_values, d_skip, cellCount, d_geneIdOfIndex, indexCount,
                              d_outToc, d_outData, d_outCells, stream);
}

void em2_set_ingest_lds_row_limit(uint32_t entries)
{
    em2::ldsRowLimitSetting.store(entries > em2::kMaxLdsRowLimit ? em2::kMaxLdsRowLimit : entries);
}

}  // extern "C"
