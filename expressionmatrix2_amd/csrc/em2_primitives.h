// em2_primitives.h -- the device-wide sorts, scans and reductions of the drivers, one function per combination of types
// that a driver uses; em2_primitives.hip, the only file that names rocPRIM, instantiates each once for the whole library.
//
// Every operation is a pair: <operation>Bytes(...) gives the bytes of temporary device memory that a run of that size and
// bit range needs (it launches nothing and builds the null arguments of rocPRIM's size query itself), and the run takes that
// memory as (temp, bytes).  The two must be given the same count and the same bit range.  All runs are asynchronous on `stream`.
// A size query takes no stream: it asks on the null stream, so the configuration behind its answer is the current device's,
// and a run's stream has to belong to the device that was current at the query (every caller's does).
//
// Radix sorts order by the key's bits [beginBit, endBit) and are stable.  Two forms, which differ in the temporary memory they
// need and in what becomes of the input:
//   * in/out         (in, out): `in` is left as it was, `out` holds the result;
//   * double buffer  DoubleBuffer<T>{current, alternate}: both arrays are scratch; afterwards current() is the one that holds
//                    the result and alternate() the other (its content is unspecified).
#ifndef EM2_PRIMITIVES_H
#define EM2_PRIMITIVES_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace em2 {

template <class T> struct DoubleBuffer {
    T* buffers[2];
    T* current() const { return buffers[0]; }
    T* alternate() const { return buffers[1]; }
};

// ---- radix sort of 64-bit keys ----
hipError_t sortKeysBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);               // in/out
hipError_t sortKeysBufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);         // double buffer
hipError_t sortKeys(void* temp, size_t bytes, const uint64_t* in, uint64_t* out, size_t count, unsigned beginBit, unsigned endBit,
                    hipStream_t stream);
hipError_t sortKeys(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, size_t count, unsigned beginBit, unsigned endBit,
                    hipStream_t stream);

// ---- radix sort of (key, value) pairs; the size queries are named after the two types ----
hipError_t sortPairsU64U32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);        // in/out
hipError_t sortPairsU64U32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);  // double buffer
hipError_t sortPairsU64F32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);        // in/out
hipError_t sortPairsU64F32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);  // double buffer
hipError_t sortPairsU32U32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);        // in/out
hipError_t sortPairsU32F32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes);  // double buffer
hipError_t sortPairs(void* temp, size_t bytes, const uint64_t* keysIn, uint64_t* keysOut, const uint32_t* valuesIn, uint32_t* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream);
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, DoubleBuffer<uint32_t>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream);
hipError_t sortPairs(void* temp, size_t bytes, const uint64_t* keysIn, uint64_t* keysOut, const float* valuesIn, float* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream);
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, DoubleBuffer<float>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream);
hipError_t sortPairs(void* temp, size_t bytes, const uint32_t* keysIn, uint32_t* keysOut, const uint32_t* valuesIn, uint32_t* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream);
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint32_t>& keys, DoubleBuffer<float>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream);

// ---- segmented radix sort of 32-bit keys, in/out: segment s is [beginOffsets[s], endOffsets[s]) ----
hipError_t segmentedSortKeysBytes(unsigned count, unsigned segments, unsigned beginBit, unsigned endBit, size_t& bytes);
hipError_t segmentedSortKeys(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, unsigned count, unsigned segments,
                             const uint32_t* beginOffsets, const uint32_t* endOffsets, unsigned beginBit, unsigned endBit,
                             hipStream_t stream);

// ---- sums of counts, added in the type of `out`: out[i] = in[0] + ... + in[i - 1] (exclusive) or ... + in[i] (inclusive) ----
hipError_t exclusiveScanU32ToU64Bytes(size_t count, size_t& bytes);
hipError_t exclusiveScanU64Bytes(size_t count, size_t& bytes);
hipError_t exclusiveScanU32Bytes(size_t count, size_t& bytes);
hipError_t inclusiveScanBytes(size_t count, size_t& bytes);                                              // 32-bit to 32-bit
hipError_t exclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint64_t* out, size_t count, hipStream_t stream);
hipError_t exclusiveScan(void* temp, size_t bytes, const uint64_t* in, uint64_t* out, size_t count, hipStream_t stream);
hipError_t exclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream);
hipError_t inclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream);

// ---- *out = the largest of in[count], 0 where count == 0 ----
hipError_t reduceMaxBytes(size_t count, size_t& bytes);
hipError_t reduceMax(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream);

}  // namespace em2

#endif
