// em2_csv.hip -- the device pass over the text of an expression counts file (the per-line work of ExpressionMatrix::addCells,
// src/ExpressionMatrix.cpp:559-626: getline, tokenize, strtof per kept field): em2_dev_csv_parse, and the session that keeps
// the decided counts of all chunks on the device, sorts them by (cell, line) and hands the CSR to em2_dev_ingest_count / _fill.
//
//   csvCountKernel    a workgroup per tile of the text, 16-byte loads: the '\n' bytes of the tile
//   (em2_primitives)  exclusive scan of the tiles' counts: the line number at which each tile starts
//   csvLinesKernel    the same read once more: the offset of the '\n' that ends line i, and the lines that hold a '\\'
//   csvFieldsKernel   a wave per line, 64 bytes per step, a byte per lane: the ballots of '"' and separator bytes, the quote
//                     state as a prefix XOR over the quote ballot, the separators outside quotes; the lane that owns the byte
//                     ending a field knows the field's start (the separator before it) and its column (the separators before
//                     it), and decides the field or defers it; the decided counts are staged in LDS, 512 per wave, and
//                     appended to the list in one piece
//
// Lines are getline's: they end at '\n' whatever the quotes say, so the quote state never crosses a line and no scan over
// tiles carries it.  A kernel never forms an address from file content: every offset is a position of the walk itself,
// below the text's length, and every index into an output is checked against its capacity.
//
// A field is decided only where strtof's bits are proven (include/em2_lsh.h, em2_dev_csv_parse); everything else is deferred
// to the host, which has the box's strtof.
#include "em2_csv.h"
#include "em2_entry.h"
#include "em2_primitives.h"
#include "em2_scratch.h"
#include "em2_wave.h"

#include <cstring>

#include <atomic>
#include <memory>
#include <string>

using namespace em2::entry;

namespace em2 {

namespace {

constexpr uint32_t kDefaultTileBytes = 16384;
constexpr uint32_t kMaxTileBytes = 1u << 20;
constexpr uint32_t kMaxFieldBytes = 32;                    // a longer trimmed field is deferred
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kMaxTextBytes = 0xf0000000u;

std::atomic<uint32_t> tileBytesSetting{0};

__device__ const double kPow10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                                      1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};

// The 16 bytes at positions [word, word + 16) of the aligned space (position = offset into the text + misalign); bytes
// outside the text read as 0, which is none of the bytes looked for.
__device__ __forceinline__ void loadWord(const uint8_t* __restrict__ text, uint32_t n, uint32_t misalign, uint64_t word, uint8_t (&bytes)[16])
{
    if (word >= misalign && word - misalign + 16u <= n) {
        const uint4 v = *reinterpret_cast<const uint4*>(text + (word - misalign));
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; j++) bytes[j] = uint8_t(w[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t at = word + uint32_t(j);
            bytes[j] = at >= misalign && at - misalign < n ? text[at - misalign] : uint8_t(0);
        }
    }
}

__global__ __launch_bounds__(256) void csvCountKernel(const uint8_t* __restrict__ text, uint32_t n, uint32_t misalign, uint32_t tileBytes,
                                                      uint32_t tileCount, uint32_t* __restrict__ newlinesOfTile)
{
    __shared__ uint32_t total;
    for (uint32_t tile = blockIdx.x; tile < tileCount; tile += gridDim.x) {
        if (threadIdx.x == 0) total = 0;
        __syncthreads();
        uint32_t count = 0;
        for (uint32_t at = threadIdx.x * 16u; at < tileBytes; at += 256u * 16u) {
            uint8_t bytes[16];
            loadWord(text, n, misalign, uint64_t(tile) * tileBytes + at, bytes);
#pragma unroll
            for (int j = 0; j < 16; j++) count += bytes[j] == '\n' ? 1u : 0u;
        }
        if (count) atomicAdd(&total, count);
        __syncthreads();
        if (threadIdx.x == 0) newlinesOfTile[tile] = total;
        __syncthreads();
    }
}

// [0] the '\n' bytes of the text, [1] its lines (a last line without '\n' counts).
__global__ void csvTotalKernel(const uint8_t* text, uint32_t n, const uint32_t* newlinesOfTile, const uint32_t* firstLineOfTile,
                               uint32_t tileCount, uint32_t* totals)
{
    const uint32_t newlines = tileCount ? firstLineOfTile[tileCount - 1u] + newlinesOfTile[tileCount - 1u] : 0u;
    totals[0] = newlines;
    totals[1] = newlines + (n && text[n - 1u] != '\n' ? 1u : 0u);
}

__global__ __launch_bounds__(256) void csvLinesKernel(const uint8_t* __restrict__ text, uint32_t n, uint32_t misalign, uint32_t tileBytes,
                                                      uint32_t tileCount, const uint32_t* __restrict__ firstLineOfTile, uint32_t lineCount,
                                                      uint32_t* __restrict__ newlineOfLine, uint8_t* __restrict__ escapeOfLine)
{
    __shared__ uint32_t waveTotals[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t tile = blockIdx.x; tile < tileCount; tile += gridDim.x) {
        uint32_t running = firstLineOfTile[tile];
        for (uint32_t step = 0; step < tileBytes; step += 256u * 16u) {
            const uint32_t at = step + threadIdx.x * 16u;
            uint8_t bytes[16];
            uint32_t count = 0;
            if (at < tileBytes) {
                loadWord(text, n, misalign, uint64_t(tile) * tileBytes + at, bytes);
#pragma unroll
                for (int j = 0; j < 16; j++) count += bytes[j] == '\n' ? 1u : 0u;
            }
            const uint32_t inclusive = waveInclusiveScan(count);
            if (lane == 63u) waveTotals[wave] = inclusive;
            __syncthreads();
            uint32_t line = running + inclusive - count, stepTotal = 0;
            for (uint32_t w = 0; w < 4u; w++) {
                if (w < wave) line += waveTotals[w];
                stepTotal += waveTotals[w];
            }
            __syncthreads();
            running += stepTotal;
            if (at < tileBytes) {
                const uint64_t position = uint64_t(tile) * tileBytes + at;       // bytes outside the text are 0: neither is met there
#pragma unroll
                for (int j = 0; j < 16; j++) {
                    if (bytes[j] == '\\' && line < lineCount) escapeOfLine[line] = 1;
                    if (bytes[j] == '\n') {
                        if (line < lineCount) newlineOfLine[line] = uint32_t(position + uint32_t(j) - misalign);
                        line++;
                    }
                }
            }
        }
    }
}

struct FieldArguments {
    const uint8_t* text;
    uint32_t n;
    const uint32_t* newlineOfLine;
    const uint8_t* escapeOfLine;
    uint32_t newlineCount, lineCount;
    uint64_t separators;                                    // separatorCount bytes
    uint32_t separatorCount;
    uint32_t expectedTokens;
    const uint32_t* keptCellOfColumn;                       // [expectedTokens]
    uint32_t lineBase;
    uint32_t* lineTable;                                    // 6 per line
    uint64_t tripleCapacity;
    uint64_t* tripleKeys;
    float* tripleValues;
    uint64_t deferredCapacity;
    uint32_t* deferred;                                     // 4 per field
    unsigned long long* counters;                           // [0] triples, [1] deferred fields
};

__device__ __forceinline__ bool isBlank(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }
__device__ __forceinline__ bool isDigit(uint8_t c) { return c >= '0' && c <= '9'; }

// The count of the field [begin, end) of a kept column.  0: skipped ("0", "0."); 1: *value is strtof's; 2: deferred.
__device__ int decideField(const uint8_t* __restrict__ text, uint32_t begin, uint32_t end, float* value)
{
    while (begin < end && isBlank(text[begin])) begin++;
    while (end > begin && isBlank(text[end - 1u])) end--;
    const uint32_t length = end - begin;
    if (length == 0 || length > kMaxFieldBytes) return 2;
    if (text[begin] == '0' && (length == 1u || (length == 2u && text[begin + 1u] == '.'))) return 0;
    uint32_t i = begin;
    bool negative = false;
    if (text[i] == '+' || text[i] == '-') {
        negative = text[i] == '-';
        i++;
    }
    uint64_t m = 0;
    uint32_t significant = 0;
    int fractionDigits = 0;
    bool anyDigit = false;
    for (; i < end && isDigit(text[i]); i++) {
        const uint32_t digit = text[i] - '0';
        anyDigit = true;
        if (m || digit) {
            if (++significant > 19u) return 2;
            m = m * 10u + digit;
        }
    }
    if (i < end && text[i] == '.') {
        for (i++; i < end && isDigit(text[i]); i++) {
            const uint32_t digit = text[i] - '0';
            anyDigit = true;
            fractionDigits++;
            if (m || digit) {
                if (++significant > 19u) return 2;
                m = m * 10u + digit;
            }
        }
    }
    if (!anyDigit) return 2;
    int exponent = 0;
    if (i < end && (text[i] == 'e' || text[i] == 'E')) {
        i++;
        bool negativeExponent = false;
        if (i < end && (text[i] == '+' || text[i] == '-')) {
            negativeExponent = text[i] == '-';
            i++;
        }
        uint32_t exponentDigits = 0;
        for (; i < end && isDigit(text[i]); i++) {
            if (++exponentDigits > 4u) return 2;
            exponent = exponent * 10 + int(text[i] - '0');
        }
        if (exponentDigits == 0) return 2;
        if (negativeExponent) exponent = -exponent;
    }
    if (i != end) return 2;                                                   // anything else: a quote, hex, trailing text
    if (m > (uint64_t(1) << 53)) return 2;
    const int q = exponent - fractionDigits;
    if (q < -22 || q > 22) return 2;
    // exact operands, one correctly rounded operation: d is the double nearest the field's value
    const double d = q >= 0 ? __dmul_rn(double(m), kPow10[q]) : __ddiv_rn(double(m), kPow10[-q]);
    if ((uint64_t(__double_as_longlong(d)) & 0x1fffffffull) == 0x10000000ull) return 2;       // a float midpoint: either side
    if (d != 0. && (d < 0x1p-126 || d > 0x1p127)) return 2;
    const float f = __double2float_rn(d);
    *value = negative ? -f : f;
    return 1;
}

__device__ __forceinline__ uint64_t prefixXor(uint64_t x)
{
    x ^= x << 1;
    x ^= x << 2;
    x ^= x << 4;
    x ^= x << 8;
    x ^= x << 16;
    x ^= x << 32;
    return x;
}

// The slot of this lane among `mask`'s lanes in a list that grows by the wave's share at once.
__device__ __forceinline__ uint64_t appendSlot(unsigned long long* counter, uint64_t mask, uint32_t lane)
{
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    const uint32_t low = __shfl(uint32_t(base), 0, 64), high = __shfl(uint32_t(base >> 32), 0, 64);
    return ((uint64_t(high) << 32) | low) + lanesBelow(mask);
}

// The wave's staged counts go to the list in one piece: one atomic on the list's counter per kStaged counts, not one per
// step of every wave (all on one address: measured, 39 ms of a 40 ms pass over 256 MB).
constexpr uint32_t kStaged = 512;

__device__ __forceinline__ void flushStaged(const FieldArguments& a, const uint64_t* keys, const float* values, uint32_t staged, uint32_t lane)
{
    waveSync();
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(&a.counters[0], (unsigned long long)staged);
    const uint32_t low = __shfl(uint32_t(base), 0, 64), high = __shfl(uint32_t(base >> 32), 0, 64);
    const uint64_t first = (uint64_t(high) << 32) | low;
    for (uint32_t i = lane; i < staged; i += 64u) {
        if (first + i < a.tripleCapacity) {
            a.tripleKeys[first + i] = keys[i];
            a.tripleValues[first + i] = values[i];
        }
    }
    waveSync();
}

__global__ __launch_bounds__(256) void csvFieldsKernel(const FieldArguments a)
{
    __shared__ uint64_t stagedKeys[4][kStaged];
    __shared__ float stagedValues[4][kStaged];
    const uint32_t lane = threadIdx.x & 63u;
    uint64_t* myKeys = stagedKeys[threadIdx.x >> 6];
    float* myValues = stagedValues[threadIdx.x >> 6];
    uint32_t staged = 0;
    for (uint64_t l = uint64_t(blockIdx.x) * 4u + (threadIdx.x >> 6); l < a.lineCount; l += uint64_t(gridDim.x) * 4u) {
        const uint32_t line = uint32_t(l);
        const uint32_t begin = line ? a.newlineOfLine[line - 1u] + 1u : 0u;
        const uint32_t rawEnd = line < a.newlineCount ? a.newlineOfLine[line] : a.n;
        if (begin > rawEnd || rawEnd > a.n) continue;                         // (never: the offsets are this pass's own)
        uint32_t end = rawEnd;
        if (end > begin && a.text[end - 1u] == '\r') end--;
        uint32_t status = kNone, tokenCount = 0;
        if (a.escapeOfLine[line]) status = host::kCsvEscape;
        else if (rawEnd == begin) status = host::kCsvEmpty;
        const bool walked = status == kNone && end > begin;                   // then column 0 has a lane that closes it
        if (lane == 0 && !walked) {
            a.lineTable[size_t(line) * 6u + 4u] = begin;
            a.lineTable[size_t(line) * 6u + 5u] = begin;
        }
        if (walked) {
            bool inQuote = false;
            uint32_t fieldBegin = begin;
            for (uint64_t base = begin; base <= end; base += 64u) {
                const uint64_t position = base + lane;
                const bool valid = position < end;
                const uint8_t c = valid ? a.text[position] : uint8_t(0);
                bool separator = false;
                for (uint32_t k = 0; k < a.separatorCount; k++) separator = separator || c == uint8_t(a.separators >> (8u * k));
                const uint64_t quotes = __ballot(valid && c == '"');
                const uint64_t inside = prefixXor(quotes) ^ (inQuote ? ~uint64_t(0) : uint64_t(0));
                const uint64_t closers = (__ballot(valid && separator) & ~inside) | __ballot(position == end);
                const uint64_t below = closers & ((uint64_t(1) << lane) - 1u);
                int kind = -1;
                float value = 0.f;
                uint32_t column = 0, myBegin = 0;
                if ((closers >> lane) & 1u) {
                    column = tokenCount + uint32_t(__popcll(below));
                    myBegin = below ? uint32_t(base) + (63u - uint32_t(__clzll(below))) + 1u : fieldBegin;
                    if (column == 0) {
                        a.lineTable[size_t(line) * 6u + 4u] = myBegin;
                        a.lineTable[size_t(line) * 6u + 5u] = uint32_t(position);
                    }
                    if (column < a.expectedTokens && a.keptCellOfColumn[column] != kNone) {
                        kind = decideField(a.text, myBegin, uint32_t(position), &value);
                    }
                }
                const uint64_t emitted = __ballot(kind == 1), deferred = __ballot(kind == 2);
                if (emitted) {
                    if (staged + uint32_t(__popcll(emitted)) > kStaged) {
                        flushStaged(a, myKeys, myValues, staged, lane);
                        staged = 0;
                    }
                    if (kind == 1) {
                        const uint32_t slot = staged + lanesBelow(emitted);       // below kStaged: at most 64 join per step
                        myKeys[slot] = (uint64_t(a.keptCellOfColumn[column]) << 32) | (a.lineBase + line);
                        myValues[slot] = value;
                    }
                    staged += uint32_t(__popcll(emitted));
                }
                if (deferred) {
                    const uint64_t slot = appendSlot(&a.counters[1], deferred, lane);
                    if (kind == 2 && slot < a.deferredCapacity) {
                        uint32_t* out = a.deferred + slot * 4u;
                        out[0] = a.lineBase + line;
                        out[1] = column;
                        out[2] = myBegin;
                        out[3] = uint32_t(position);
                    }
                }
                inQuote = inQuote != ((__popcll(quotes) & 1) != 0);
                tokenCount += uint32_t(__popcll(closers));
                if (closers) fieldBegin = uint32_t(base) + (63u - uint32_t(__clzll(closers))) + 1u;
            }
        }
        if (status == kNone) status = tokenCount == a.expectedTokens ? uint32_t(host::kCsvOk) : uint32_t(host::kCsvTokenCount);
        if (lane == 0) {
            uint32_t* out = a.lineTable + size_t(line) * 6u;
            out[0] = begin;
            out[1] = end;
            out[2] = tokenCount;
            out[3] = status;
        }
    }
    if (staged) flushStaged(a, myKeys, myValues, staged, lane);
}

uint32_t tileBytesNow()
{
    const uint32_t setting = tileBytesSetting.load();
    return setting ? setting : kDefaultTileBytes;
}

// counts: [0] lines, [1] triples, [2] deferred fields.
hipError_t runParse(const uint8_t* d_text, uint32_t n, uint64_t separators, uint32_t separatorCount, uint32_t expectedTokens,
                    const uint32_t* d_keptCellOfColumn, uint32_t lineBase, uint32_t lineCapacity, uint32_t* d_lineTable,
                    uint64_t tripleCapacity, uint64_t* d_tripleKeys, float* d_tripleValues, uint64_t deferredCapacity, uint32_t* d_deferred,
                    uint64_t* counts, hipStream_t stream)
{
    counts[0] = counts[1] = counts[2] = 0;
    if (n == 0) return hipSuccess;
    const uint32_t tileBytes = tileBytesNow();
    const uint32_t misalign = uint32_t(reinterpret_cast<uintptr_t>(d_text) & 15u);
    const uint32_t tileCount = uint32_t((uint64_t(n) + misalign + tileBytes - 1u) / tileBytes);
    const uint32_t tileBlocks = tileCount < 65536u ? tileCount : 65536u;
    DeviceBuffer newlinesOfTile, firstLineOfTile, totals, scanTemp, newlineOfLine, escapeOfLine, counters;
    EM2_TRY(newlinesOfTile.allocate(size_t(tileCount) * sizeof(uint32_t)));
    EM2_TRY(firstLineOfTile.allocate(size_t(tileCount) * sizeof(uint32_t)));
    EM2_TRY(totals.allocate(2u * sizeof(uint32_t)));
    csvCountKernel<<<dim3(tileBlocks), dim3(256), 0, stream>>>(d_text, n, misalign, tileBytes, tileCount, newlinesOfTile.as<uint32_t>());
    EM2_TRY(hipGetLastError());
    size_t tempBytes = 0;
    EM2_TRY(exclusiveScanU32Bytes(size_t(tileCount), tempBytes));
    EM2_TRY(scanTemp.allocate(tempBytes));
    EM2_TRY(exclusiveScan(scanTemp.p, tempBytes, newlinesOfTile.as<uint32_t>(), firstLineOfTile.as<uint32_t>(), size_t(tileCount), stream));
    csvTotalKernel<<<dim3(1), dim3(1), 0, stream>>>(d_text, n, newlinesOfTile.as<uint32_t>(), firstLineOfTile.as<uint32_t>(), tileCount,
                                                    totals.as<uint32_t>());
    EM2_TRY(hipGetLastError());
    uint32_t hostTotals[2] = {0, 0};
    EM2_TRY(hipMemcpyAsync(hostTotals, totals.p, sizeof(hostTotals), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    const uint32_t lineCount = hostTotals[1];
    counts[0] = lineCount;
    if (lineCount > lineCapacity) return hipSuccess;

    EM2_TRY(newlineOfLine.allocate(size_t(lineCount) * sizeof(uint32_t)));
    EM2_TRY(escapeOfLine.allocate(lineCount));
    EM2_TRY(counters.allocate(2u * sizeof(unsigned long long)));
    EM2_TRY(hipMemsetAsync(newlineOfLine.p, 0, size_t(lineCount) * sizeof(uint32_t), stream));
    EM2_TRY(hipMemsetAsync(escapeOfLine.p, 0, lineCount, stream));
    EM2_TRY(hipMemsetAsync(counters.p, 0, 2u * sizeof(unsigned long long), stream));
    csvLinesKernel<<<dim3(tileBlocks), dim3(256), 0, stream>>>(d_text, n, misalign, tileBytes, tileCount, firstLineOfTile.as<uint32_t>(),
                                                               lineCount, newlineOfLine.as<uint32_t>(), escapeOfLine.as<uint8_t>());
    EM2_TRY(hipGetLastError());
    FieldArguments a{};
    a.text = d_text;
    a.n = n;
    a.newlineOfLine = newlineOfLine.as<uint32_t>();
    a.escapeOfLine = escapeOfLine.as<uint8_t>();
    a.newlineCount = hostTotals[0];
    a.lineCount = lineCount;
    a.separators = separators;
    a.separatorCount = separatorCount;
    a.expectedTokens = expectedTokens;
    a.keptCellOfColumn = d_keptCellOfColumn;
    a.lineBase = lineBase;
    a.lineTable = d_lineTable;
    a.tripleCapacity = tripleCapacity;
    a.tripleKeys = d_tripleKeys;
    a.tripleValues = d_tripleValues;
    a.deferredCapacity = deferredCapacity;
    a.deferred = d_deferred;
    a.counters = counters.as<unsigned long long>();
    const uint32_t fieldBlocks = (lineCount + 3u) / 4u;
    csvFieldsKernel<<<dim3(fieldBlocks < 16384u ? fieldBlocks : 16384u), dim3(256), 0, stream>>>(a);
    EM2_TRY(hipGetLastError());
    unsigned long long hostCounters[2] = {0, 0};
    EM2_TRY(hipMemcpyAsync(hostCounters, counters.p, sizeof(hostCounters), hipMemcpyDeviceToHost, stream));
    EM2_TRY(hipStreamSynchronize(stream));
    counts[1] = hostCounters[0];
    counts[2] = hostCounters[1];
    return hipSuccess;
}

int devCsvParse(const char* who, const char* d_text, uint64_t textBytes, const char* separators, uint32_t separatorCount,
                uint32_t expectedTokens, const uint32_t* d_keptCellOfColumn, uint32_t lineBase, uint32_t lineCapacity, uint32_t* d_lineTable,
                uint64_t tripleCapacity, uint64_t* d_tripleKeys, float* d_tripleValues, uint64_t deferredCapacity, uint32_t* d_deferred,
                uint64_t* counts, void* stream)
{
    if (!counts || !separators || (textBytes && !d_text) || (expectedTokens && !d_keptCellOfColumn) || (lineCapacity && !d_lineTable) ||
        (tripleCapacity && (!d_tripleKeys || !d_tripleValues)) || (deferredCapacity && !d_deferred)) {
        return failNull(who);
    }
    if (!host::csvSeparatorsRunOnDevice(std::string(separators, separatorCount))) {
        return fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the device takes 1 to 8 separator bytes, none of them '\"', '\\', "
                                                                       "a line feed, a carriage return or NUL");
    }
    if (textBytes > kMaxTextBytes) return failArgument(who, "a chunk is at most 0xf0000000 bytes");
    if (!haveDevice()) return failNoDevice(who);
    uint64_t packed = 0;
    for (uint32_t k = 0; k < separatorCount; k++) packed |= uint64_t(uint8_t(separators[k])) << (8u * k);
    EM2_HIP_FOR(who, runParse(reinterpret_cast<const uint8_t*>(d_text), uint32_t(textBytes), packed, separatorCount, expectedTokens,
                              d_keptCellOfColumn, lineBase, lineCapacity, d_lineTable, tripleCapacity, d_tripleKeys, d_tripleValues,
                              deferredCapacity, d_deferred, counts, static_cast<hipStream_t>(stream)));
    return EM2_OK;
}

// key in: cell << 32 | line; out: cell << lineBits | line.
__global__ void csvPackKeysKernel(uint64_t* keys, uint64_t count, uint32_t lineBits)
{
    for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        const uint64_t key = keys[i];
        keys[i] = ((key >> 32) << lineBits) | (key & 0xffffffffull);
    }
}

// indptr[c]: the first sorted key whose cell part is not below c; indptr[cellCount] = count.
__global__ void csvIndptrKernel(const uint64_t* __restrict__ keys, uint64_t count, uint32_t lineBits, uint32_t cellCount, uint64_t* indptr)
{
    for (uint64_t c = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; c <= cellCount; c += uint64_t(gridDim.x) * blockDim.x) {
        uint64_t low = 0, high = count;
        while (low < high) {
            const uint64_t middle = low + (high - low) / 2u;
            if ((keys[middle] >> lineBits) < c) low = middle + 1u;
            else high = middle;
        }
        indptr[c] = low;
    }
}

__global__ void csvIndicesKernel(const uint64_t* __restrict__ keys, uint64_t count, uint32_t lineBits, uint32_t* __restrict__ indices)
{
    const uint64_t mask = (uint64_t(1) << lineBits) - 1u;
    for (uint64_t i = blockIdx.x * uint64_t(blockDim.x) + threadIdx.x; i < count; i += uint64_t(gridDim.x) * blockDim.x) {
        indices[i] = uint32_t(keys[i] & mask);
    }
}

uint32_t bitsFor(uint32_t count)                           // the bits that hold every value below count, at least 1
{
    uint32_t bits = 1;
    while (bits < 32u && (uint64_t(1) << bits) < count) bits++;
    return bits;
}

struct Scratch : CachedBuffer {                            // every call here ends with the stream synchronised
    Scratch() { idle = true; }
};

}  // namespace

namespace host {

struct CsvSession {
    struct Part {
        std::unique_ptr<Scratch> keys, values;
        uint64_t count = 0;
    };
    std::vector<Part> parts;
};

CsvSession* csvSessionCreate() { return new CsvSession; }
void csvSessionDestroy(CsvSession* session) { delete session; }

int csvSessionChunk(CsvSession* session, const char* text, uint64_t bytes, const std::string& separators, uint32_t expectedTokens,
                    const std::vector<uint32_t>& keptCellOfColumn, uint32_t lineBase, std::vector<CsvLine>& lines,
                    std::vector<CsvDeferred>& deferred)
{
    const char* who = "em2_matrix_add_cells_csv";
    lines.clear();
    deferred.clear();
    if (!haveDevice()) return failNoDevice(who);
    if (bytes == 0) return EM2_OK;
    Scratch dText;
    DeviceBuffer dKept, dLines, dDeferred;
    EM2_HIP_FOR(who, dText.allocate(size_t(bytes)));
    EM2_HIP_FOR(who, hipMemcpy(dText.p, text, size_t(bytes), hipMemcpyHostToDevice));
    EM2_HIP_FOR(who, dKept.upload(keptCellOfColumn.data(), keptCellOfColumn.size()));
    // A line that passes has at least expectedTokens bytes with its '\n'; shorter ones, a first guess for the counts of a
    // file that is mostly "0", and a first guess for the deferred fields are put right by a second run with what the first
    // one counted.
    uint64_t lineCapacity = bytes / expectedTokens + 2u, tripleCapacity = bytes / 8u + 1024u, deferredCapacity = bytes / 64u + 1024u;
    CsvSession::Part part;
    uint64_t counts[3] = {0, 0, 0};
    for (int attempt = 0;; attempt++) {
        part.keys.reset(new Scratch);
        part.values.reset(new Scratch);
        EM2_HIP_FOR(who, part.keys->allocate(size_t(tripleCapacity) * sizeof(uint64_t)));
        EM2_HIP_FOR(who, part.values->allocate(size_t(tripleCapacity) * sizeof(float)));
        EM2_HIP_FOR(who, dLines.allocateFor<CsvLine>(size_t(lineCapacity)));
        EM2_HIP_FOR(who, dDeferred.allocateFor<CsvDeferred>(size_t(deferredCapacity)));
        const int rc = devCsvParse(who, static_cast<const char*>(dText.p), bytes, separators.data(), uint32_t(separators.size()),
                                   expectedTokens, dKept.as<uint32_t>(), lineBase, uint32_t(lineCapacity), dLines.as<uint32_t>(),
                                   tripleCapacity, part.keys->as<uint64_t>(), part.values->as<float>(), deferredCapacity,
                                   dDeferred.as<uint32_t>(), counts, nullptr);
        if (rc != EM2_OK) return rc;
        if (counts[0] <= lineCapacity && counts[1] <= tripleCapacity && counts[2] <= deferredCapacity) break;
        if (attempt == 2) return fail(EM2_ERROR_RUNTIME, std::string(who) + ": the device pass does not settle on its counts");
        if (counts[0] > lineCapacity) {                                       // (the fields were not read yet)
            lineCapacity = counts[0];
        } else {
            tripleCapacity = counts[1] > tripleCapacity ? counts[1] : tripleCapacity;
            deferredCapacity = counts[2] > deferredCapacity ? counts[2] : deferredCapacity;
        }
    }
    if (uint64_t(lineBase) + counts[0] >= kNone) return fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": too many lines");
    lines.resize(size_t(counts[0]));
    deferred.resize(size_t(counts[2]));
    EM2_HIP_FOR(who, dLines.download(lines.data(), lines.size()));
    EM2_HIP_FOR(who, dDeferred.download(deferred.data(), deferred.size()));
    part.count = counts[1];
    session->parts.push_back(std::move(part));
    return EM2_OK;
}

int csvSessionFinish(CsvSession* session, const std::vector<CsvTriple>& extra, uint32_t keptCellCount, uint32_t lineCount,
                     const std::vector<uint32_t>& geneIdOfLine, std::vector<uint32_t>& status, std::vector<uint64_t>& toc,
                     std::vector<em2_count>& data, std::vector<CellRecord>& cells, bool* failed)
{
    const char* who = "em2_matrix_add_cells_csv";
    *failed = false;
    status.assign(keptCellCount, 0u);
    toc.assign(size_t(keptCellCount) + 1u, 0u);
    data.clear();
    cells.assign(keptCellCount, CellRecord());
    if (keptCellCount == 0) return EM2_OK;
    if (!haveDevice()) return failNoDevice(who);
    uint64_t total = extra.size();
    for (const CsvSession::Part& part : session->parts) total += part.count;

    // One list of all counts, sorted by cell << bits(lines) | line over exactly the live bits: the keys are unique, so the
    // order in which the lanes and the host appended them cannot show.
    const uint32_t lineBits = bitsFor(lineCount), cellBits = bitsFor(keptCellCount);
    Scratch keysIn, keysOut, valuesIn, valuesOut, sortTemp, dIndices;
    DeviceBuffer dIndptr, dGenes, dKept, dStatus, dDuplicate, dToc, dData, dCells;
    EM2_HIP_FOR(who, keysIn.allocate(size_t(total) * sizeof(uint64_t)));
    EM2_HIP_FOR(who, keysOut.allocate(size_t(total) * sizeof(uint64_t)));
    EM2_HIP_FOR(who, valuesIn.allocate(size_t(total) * sizeof(float)));
    EM2_HIP_FOR(who, valuesOut.allocate(size_t(total) * sizeof(float)));
    EM2_HIP_FOR(who, dIndices.allocate(size_t(total) * sizeof(uint32_t)));
    uint64_t at = 0;
    for (CsvSession::Part& part : session->parts) {
        if (part.count) {
            EM2_HIP_FOR(who, hipMemcpy(keysIn.as<uint64_t>() + at, part.keys->p, size_t(part.count) * sizeof(uint64_t), hipMemcpyDeviceToDevice));
            EM2_HIP_FOR(who, hipMemcpy(valuesIn.as<float>() + at, part.values->p, size_t(part.count) * sizeof(float), hipMemcpyDeviceToDevice));
        }
        at += part.count;
        part.keys.reset();
        part.values.reset();
    }
    session->parts.clear();
    if (!extra.empty()) {
        std::vector<uint64_t> keys(extra.size());
        std::vector<float> values(extra.size());
        for (size_t i = 0; i < extra.size(); i++) {
            if (extra[i].cell >= keptCellCount || extra[i].line >= lineCount) {
                return failArgument(who, "a count of the host names no kept cell or no line");
            }
            keys[i] = (uint64_t(extra[i].cell) << 32) | extra[i].line;
            values[i] = extra[i].value;
        }
        EM2_HIP_FOR(who, hipMemcpy(keysIn.as<uint64_t>() + at, keys.data(), keys.size() * sizeof(uint64_t), hipMemcpyHostToDevice));
        EM2_HIP_FOR(who, hipMemcpy(valuesIn.as<float>() + at, values.data(), values.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    EM2_HIP_FOR(who, dIndptr.allocateFor<uint64_t>(size_t(keptCellCount) + 1u));
    const uint64_t* sortedKeys = keysIn.as<uint64_t>();
    const float* sortedValues = valuesIn.as<float>();
    if (total) {
        csvPackKeysKernel<<<dim3(gridFor(total)), dim3(256)>>>(keysIn.as<uint64_t>(), total, lineBits);
        EM2_HIP_FOR(who, hipGetLastError());
        size_t tempBytes = 0;
        EM2_HIP_FOR(who, sortPairsU64F32Bytes(size_t(total), 0u, lineBits + cellBits, tempBytes));
        EM2_HIP_FOR(who, sortTemp.allocate(tempBytes));
        EM2_HIP_FOR(who, sortPairs(sortTemp.p, tempBytes, keysIn.as<uint64_t>(), keysOut.as<uint64_t>(), valuesIn.as<float>(), valuesOut.as<float>(),
                                   size_t(total), 0u, lineBits + cellBits, hipStream_t(nullptr)));
        sortedKeys = keysOut.as<uint64_t>();
        sortedValues = valuesOut.as<float>();
        csvIndicesKernel<<<dim3(gridFor(total)), dim3(256)>>>(sortedKeys, total, lineBits, dIndices.as<uint32_t>());
        EM2_HIP_FOR(who, hipGetLastError());
    }
    csvIndptrKernel<<<dim3(gridFor(uint64_t(keptCellCount) + 1u)), dim3(256)>>>(sortedKeys, total, lineBits, keptCellCount, dIndptr.as<uint64_t>());
    EM2_HIP_FOR(who, hipGetLastError());
    EM2_HIP_FOR(who, hipDeviceSynchronize());

    // addCell's storing part: the rows are the cells, the indices the lines, the map the ids the file's genes get.
    EM2_HIP_FOR(who, dGenes.upload(geneIdOfLine.data(), lineCount));
    EM2_HIP_FOR(who, dKept.allocateFor<uint32_t>(keptCellCount));
    EM2_HIP_FOR(who, dStatus.allocateFor<uint32_t>(keptCellCount));
    EM2_HIP_FOR(who, dDuplicate.allocateFor<uint32_t>(keptCellCount));
    EM2_HIP_FOR(who, dToc.allocateFor<uint64_t>(size_t(keptCellCount) + 1u));
    int rc = em2_dev_ingest_count(dIndptr.as<uint64_t>(), dIndices.as<uint32_t>(), sortedValues, nullptr, keptCellCount, dGenes.as<uint32_t>(),
                                  lineCount, dKept.as<uint32_t>(), dStatus.as<uint32_t>(), dDuplicate.as<uint32_t>(), dToc.as<uint64_t>(),
                                  nullptr);
    if (rc != EM2_OK) return rc;
    EM2_HIP_FOR(who, dStatus.download(status.data(), keptCellCount));
    EM2_HIP_FOR(who, dToc.download(toc.data(), size_t(keptCellCount) + 1u));
    for (uint32_t s : status) {
        if (s != 0u) *failed = true;
    }
    if (*failed) return EM2_OK;
    const uint64_t outCount = toc[keptCellCount];
    EM2_HIP_FOR(who, dData.allocateFor<em2_count>(size_t(outCount)));
    EM2_HIP_FOR(who, dCells.allocateFor<CellRecord>(keptCellCount));
    EM2_HIP_FOR(who, hipMemset(dCells.p, 0, size_t(keptCellCount) * sizeof(CellRecord)));
    rc = em2_dev_ingest_fill(dIndptr.as<uint64_t>(), dIndices.as<uint32_t>(), sortedValues, nullptr, keptCellCount, dGenes.as<uint32_t>(),
                             lineCount, dToc.as<uint64_t>(), dData.as<em2_count>(), dCells.p, nullptr);
    if (rc != EM2_OK) return rc;
    data.resize(size_t(outCount));
    EM2_HIP_FOR(who, dData.download(data.data(), size_t(outCount)));
    EM2_HIP_FOR(who, dCells.download(cells.data(), keptCellCount));
    return EM2_OK;
}

}  // namespace host
}  // namespace em2

extern "C" {

int em2_dev_csv_parse(const char* d_text, uint64_t textBytes, const char* separators, uint32_t separatorCount, uint32_t expectedTokens,
                      const uint32_t* d_keptCellOfColumn, uint32_t lineBase, uint32_t lineCapacity, uint32_t* d_lineTable,
                      uint64_t tripleCapacity, uint64_t* d_tripleKeys, float* d_tripleValues, uint64_t deferredCapacity,
                      uint32_t* d_deferred, uint64_t* counts, void* stream)
{
    return em2::devCsvParse("em2_dev_csv_parse", d_text, textBytes, separators, separatorCount, expectedTokens, d_keptCellOfColumn, lineBase,
                            lineCapacity, d_lineTable, tripleCapacity, d_tripleKeys, d_tripleValues, deferredCapacity, d_deferred, counts,
                            stream);
}

void em2_set_csv_tile_bytes(uint32_t bytes)
{
    if (bytes) {
        bytes = (bytes + 15u) & ~15u;
        if (bytes > em2::kMaxTileBytes) bytes = em2::kMaxTileBytes;
    }
    em2::tileBytesSetting.store(bytes);
}

}  // extern "C"
