// em2_chunks.h -- the chunk table of the passes that deal their work by pieces of a gene's segment of a sorted stream (device
// code): a gene's segment is cut at chunk, 2 chunk, ... FROM ITS OWN START, and chunk t of the whole problem is (gene, chunk
// within the gene), so that a gene present in every cell and a gene present in one keep the machine equally busy
// (em2_gene_information.hip, em2_rank_genes.hip).  The kernel has internal linkage: every object that includes this has its own.
#ifndef EM2_CHUNKS_H
#define EM2_CHUNKS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace em2 {
namespace {

struct ChunkRef {
    uint32_t gene;
    uint32_t index;           // the chunk's number within its gene: entries [index * chunk, + chunk) of the segment
};

// chunkStarts: the exclusive scan of the genes' chunk counts, [geneCount + 1].  A thread per chunk finds its gene: the last g
// with chunkStarts[g] <= t (genes without chunks share their start with the next gene and are passed over).
__global__ void __launch_bounds__(256)
chunkTableKernel(const uint64_t* __restrict__ chunkStarts, uint32_t geneCount, ChunkRef* __restrict__ table)
{
    const uint64_t total = chunkStarts[geneCount];
    for (uint64_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += uint64_t(gridDim.x) * blockDim.x) {
        uint32_t low = 0u, high = geneCount;               // the first g with chunkStarts[g] > t, in (0, geneCount]
        while (low < high) {
            const uint32_t middle = low + (high - low) / 2u;
            if (chunkStarts[middle] <= t) low = middle + 1u;
            else high = middle;
        }
        const uint32_t gene = low - 1u;
        table[t] = ChunkRef{gene, uint32_t(t - chunkStarts[gene])};
    }
}

}  // namespace
}  // namespace em2

#endif
