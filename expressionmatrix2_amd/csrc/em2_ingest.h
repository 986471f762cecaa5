// em2_ingest.h -- ingest: what a complete store (ExpressionMatrix::createNew, src/ExpressionMatrix.cpp:56-101) holds beyond the
// files the search paths read, and the device pass of the bulk add (em2_ingest.hip) as the host driver (em2_ingest_host.cpp)
// calls it.
//
//   GeneNames-*, CellNames-*            MemoryMapped::StringTable: gene id / cell id = string id, in order of first insertion
//   GeneMetaData.*, GeneMetaDataNames-*, GeneMetaDataValues-*, GeneMetaDataNamesUsageCount
//                                       the containers of the cell meta data (em2_meta_data.h), one list per gene
//   Cells                               MemoryMapped::Vector<Cell> (src/Cell.hpp:17-97), 56 bytes per cell
#ifndef EM2_INGEST_H
#define EM2_INGEST_H

#include "em2_host.h"
#include "em2_meta_data.h"

namespace em2 {
namespace host {

struct CellRecord {                                       // src/Cell.hpp:17-97
    double sum1, sum2, norm2, norm1Inverse, norm2Inverse, sum1LargeExpressionCounts, sum2LargeExpressionCounts;
};
static_assert(sizeof(CellRecord) == 56, "Cell layout");

// The string tables and the gene meta data live in host memory and are written back by flush(), as the cell meta data is;
// Cells grows in place, as CellExpressionCounts and the two all-sets do.
struct IngestState {
    StringTable geneNames, cellNames;
    MetaDataStore geneMetaData;
    MappedFile cells;
    bool dirty = false;                                   // the two tables of names
    std::string missing;                                  // why ingest is refused on this directory ("" = it is not)
};

// What addCell does to a cell's (gene id, count) pairs after the name look-ups (src/ExpressionMatrix.cpp:241-277), on the
// host: `entries` in the caller's order in, the kept entries ascending by gene id out.
enum { kIngestOk = 0, kIngestNegative = 1, kIngestDuplicate = 2, kIngestBadIndex = 3 };
int storeCell(std::vector<em2_count>& entries, CellRecord& cell, uint32_t& duplicateGene);

// One chunk of the bulk add on the device: uploads, em2_dev_ingest_count, and -- where every status is ok -- em2_dev_ingest_fill
// and the results back.  indptr starts at 0.  Returns an EM2 status with the last error set.  *failed = some status is not ok
// (toc, data and cells are then not filled).
int ingestChunkOnDevice(const uint64_t* indptr, const uint32_t* indices, const float* values, const uint8_t* skip, uint32_t cellCount,
                        const uint32_t* geneIdOfIndex, uint32_t indexCount, std::vector<uint32_t>& keptCount,
                        std::vector<uint32_t>& status, std::vector<uint32_t>& duplicateGene, std::vector<uint64_t>& toc,
                        std::vector<em2_count>& data, std::vector<CellRecord>& cells, bool* failed);

}  // namespace host
}  // namespace em2

#endif
