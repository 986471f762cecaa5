// em2_primitives.hip -- em2_primitives.h on rocPRIM: the one translation unit that includes it, so each sort, scan and
// reduction is compiled once for the library.  A size query is rocPRIM's own call with a null temporary pointer and null
// arrays of the run's types, which launches nothing.

#include "em2_primitives.h"

#include <cstring>      // rocprim/iterator/texture_cache_iterator.hpp calls memset without including it

#include <rocprim/rocprim.hpp>

namespace em2 {
namespace {

const hipStream_t kNoStream = nullptr;

// rocPRIM instantiates its kernels per iterator type.  The inputs go to it as plain pointers, as the double-buffer forms'
// do: a const pointer would compile a second copy of every sort kernel next to theirs.
template <class T> T* plain(const T* p) { return const_cast<T*>(p); }

template <class T> rocprim::double_buffer<T> wrap(const DoubleBuffer<T>& b) { return rocprim::double_buffer<T>(b.current(), b.alternate()); }

template <class T> void unwrap(const rocprim::double_buffer<T>& from, DoubleBuffer<T>& to)
{
    to.buffers[0] = from.current();
    to.buffers[1] = from.alternate();
}

template <class K, class V>
hipError_t pairsBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return rocprim::radix_sort_pairs(nullptr, bytes, static_cast<K*>(nullptr), static_cast<K*>(nullptr), static_cast<V*>(nullptr),
                                     static_cast<V*>(nullptr), count, beginBit, endBit, kNoStream);
}

template <class K, class V>
hipError_t pairsBufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    rocprim::double_buffer<K> keys(nullptr, nullptr);
    rocprim::double_buffer<V> values(nullptr, nullptr);
    return rocprim::radix_sort_pairs(nullptr, bytes, keys, values, count, beginBit, endBit, kNoStream);
}

template <class K, class V>
hipError_t pairs(void* temp, size_t bytes, DoubleBuffer<K>& keys, DoubleBuffer<V>& values, size_t count, unsigned beginBit,
                 unsigned endBit, hipStream_t stream)
{
    rocprim::double_buffer<K> k = wrap(keys);
    rocprim::double_buffer<V> v = wrap(values);
    const hipError_t e = rocprim::radix_sort_pairs(temp, bytes, k, v, count, beginBit, endBit, stream);
    unwrap(k, keys);
    unwrap(v, values);
    return e;
}

}  // namespace

hipError_t sortKeysBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return rocprim::radix_sort_keys(nullptr, bytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), count, beginBit,
                                    endBit, kNoStream);
}

hipError_t sortKeysBufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    rocprim::double_buffer<uint64_t> keys(nullptr, nullptr);
    return rocprim::radix_sort_keys(nullptr, bytes, keys, count, beginBit, endBit, kNoStream);
}

hipError_t sortKeys(void* temp, size_t bytes, const uint64_t* in, uint64_t* out, size_t count, unsigned beginBit, unsigned endBit,
                    hipStream_t stream)
{
    return rocprim::radix_sort_keys(temp, bytes, plain(in), out, count, beginBit, endBit, stream);
}

hipError_t sortKeys(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, size_t count, unsigned beginBit, unsigned endBit,
                    hipStream_t stream)
{
    rocprim::double_buffer<uint64_t> k = wrap(keys);
    const hipError_t e = rocprim::radix_sort_keys(temp, bytes, k, count, beginBit, endBit, stream);
    unwrap(k, keys);
    return e;
}

hipError_t sortPairsU64U32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBytes<uint64_t, uint32_t>(count, beginBit, endBit, bytes);
}
hipError_t sortPairsU64U32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBufferBytes<uint64_t, uint32_t>(count, beginBit, endBit, bytes);
}
hipError_t sortPairsU64F32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBytes<uint64_t, float>(count, beginBit, endBit, bytes);
}
hipError_t sortPairsU64F32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBufferBytes<uint64_t, float>(count, beginBit, endBit, bytes);
}
hipError_t sortPairsU32U32Bytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBytes<uint32_t, uint32_t>(count, beginBit, endBit, bytes);
}
hipError_t sortPairsU32F32BufferBytes(size_t count, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return pairsBufferBytes<uint32_t, float>(count, beginBit, endBit, bytes);
}

hipError_t sortPairs(void* temp, size_t bytes, const uint64_t* keysIn, uint64_t* keysOut, const uint32_t* valuesIn, uint32_t* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, bytes, plain(keysIn), keysOut, plain(valuesIn), valuesOut, count, beginBit, endBit, stream);
}
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, DoubleBuffer<uint32_t>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return pairs(temp, bytes, keys, values, count, beginBit, endBit, stream);
}
hipError_t sortPairs(void* temp, size_t bytes, const uint64_t* keysIn, uint64_t* keysOut, const float* valuesIn, float* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, bytes, plain(keysIn), keysOut, plain(valuesIn), valuesOut, count, beginBit, endBit, stream);
}
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint64_t>& keys, DoubleBuffer<float>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return pairs(temp, bytes, keys, values, count, beginBit, endBit, stream);
}
hipError_t sortPairs(void* temp, size_t bytes, const uint32_t* keysIn, uint32_t* keysOut, const uint32_t* valuesIn, uint32_t* valuesOut,
                     size_t count, unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return rocprim::radix_sort_pairs(temp, bytes, plain(keysIn), keysOut, plain(valuesIn), valuesOut, count, beginBit, endBit, stream);
}
hipError_t sortPairs(void* temp, size_t bytes, DoubleBuffer<uint32_t>& keys, DoubleBuffer<float>& values, size_t count,
                     unsigned beginBit, unsigned endBit, hipStream_t stream)
{
    return pairs(temp, bytes, keys, values, count, beginBit, endBit, stream);
}

hipError_t segmentedSortKeysBytes(unsigned count, unsigned segments, unsigned beginBit, unsigned endBit, size_t& bytes)
{
    return rocprim::segmented_radix_sort_keys(nullptr, bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), count,
                                              segments, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), beginBit,
                                              endBit, kNoStream);
}

hipError_t segmentedSortKeys(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, unsigned count, unsigned segments,
                             const uint32_t* beginOffsets, const uint32_t* endOffsets, unsigned beginBit, unsigned endBit,
                             hipStream_t stream)
{
    return rocprim::segmented_radix_sort_keys(temp, bytes, plain(in), out, count, segments, plain(beginOffsets), plain(endOffsets), beginBit, endBit,
                                              stream);
}

hipError_t exclusiveScanU32ToU64Bytes(size_t count, size_t& bytes)
{
    return rocprim::exclusive_scan(nullptr, bytes, static_cast<uint32_t*>(nullptr), static_cast<uint64_t*>(nullptr), uint64_t(0), count,
                                   rocprim::plus<uint64_t>(), kNoStream);
}
hipError_t exclusiveScanU64Bytes(size_t count, size_t& bytes)
{
    return rocprim::exclusive_scan(nullptr, bytes, static_cast<uint64_t*>(nullptr), static_cast<uint64_t*>(nullptr), uint64_t(0), count,
                                   rocprim::plus<uint64_t>(), kNoStream);
}
hipError_t exclusiveScanU32Bytes(size_t count, size_t& bytes)
{
    return rocprim::exclusive_scan(nullptr, bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), uint32_t(0), count,
                                   rocprim::plus<uint32_t>(), kNoStream);
}
hipError_t inclusiveScanBytes(size_t count, size_t& bytes)
{
    return rocprim::inclusive_scan(nullptr, bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), count,
                                   rocprim::plus<uint32_t>(), kNoStream);
}

hipError_t exclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint64_t* out, size_t count, hipStream_t stream)
{
    return rocprim::exclusive_scan(temp, bytes, plain(in), out, uint64_t(0), count, rocprim::plus<uint64_t>(), stream);
}
hipError_t exclusiveScan(void* temp, size_t bytes, const uint64_t* in, uint64_t* out, size_t count, hipStream_t stream)
{
    return rocprim::exclusive_scan(temp, bytes, plain(in), out, uint64_t(0), count, rocprim::plus<uint64_t>(), stream);
}
hipError_t exclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream)
{
    return rocprim::exclusive_scan(temp, bytes, plain(in), out, uint32_t(0), count, rocprim::plus<uint32_t>(), stream);
}
hipError_t inclusiveScan(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream)
{
    return rocprim::inclusive_scan(temp, bytes, plain(in), out, count, rocprim::plus<uint32_t>(), stream);
}

hipError_t reduceMaxBytes(size_t count, size_t& bytes)
{
    return rocprim::reduce(nullptr, bytes, static_cast<uint32_t*>(nullptr), static_cast<uint32_t*>(nullptr), 0u, count,
                           rocprim::maximum<uint32_t>(), kNoStream);
}
hipError_t reduceMax(void* temp, size_t bytes, const uint32_t* in, uint32_t* out, size_t count, hipStream_t stream)
{
    return rocprim::reduce(temp, bytes, plain(in), out, 0u, count, rocprim::maximum<uint32_t>(), stream);
}

}  // namespace em2
