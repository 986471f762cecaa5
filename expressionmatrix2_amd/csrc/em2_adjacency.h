// em2_adjacency.h -- the device pieces of an adjacency built by sorting: two directed records per undirected edge
// (key = vertex << 32 | neighbour), a radix sort of the keys, and a search for where every vertex's records begin.  No degree
// is counted with atomics, and within a list the neighbours ascend.  Used by em2_gene_graph.hip and em2_layout.hip.
#ifndef EM2_ADJACENCY_H
#define EM2_ADJACENCY_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace em2 {

// The first of the ascending keys[0, n) that is not below `key`, n where there is none.
__device__ __forceinline__ uint64_t lowerBound(const uint64_t* __restrict__ keys, uint64_t n, uint64_t key)
{
    uint64_t low = 0, high = n;
    while (low < high) {
        const uint64_t middle = low + (high - low) / 2u;
        if (keys[middle] < key) low = middle + 1u;
        else high = middle;
    }
    return low;
}

}  // namespace em2

#endif
