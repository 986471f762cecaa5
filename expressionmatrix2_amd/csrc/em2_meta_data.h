// em2_meta_data.h -- the cell meta data store of a data directory in the reference's file formats, and what the
// ExpressionMatrix-level meta data methods (em2_meta_data.cpp, members of em2::host::Matrix) hand to the C ABI.
//
//   CellMetaData.{toc,data,freeSlots}   MemoryMapped::VectorOfLists<pair<StringId, StringId>> (src/MemoryMappedVectorOfLists.hpp):
//                                       toc[cell] is the index of the list's end node, a node is {nameId, valueId, previous,
//                                       next} (24 bytes), a list is circular through its end node, freeSlots holds the indices
//                                       erase() gave back (the last one is reused first, :351-365).
//   CellMetaDataNames-{strings.toc,strings.data,hashTable}, CellMetaDataValues-...
//                                       MemoryMapped::StringTable<uint32_t> (src/MemoryMappedStringTable.hpp): the strings as a
//                                       VectorOfVectors<char, uint32_t>, ids in order of first insertion, and an open-addressing
//                                       table of ids (0xffffffff = empty) probed from MurmurHash64A(s, len, 237) & mask; it
//                                       doubles when strings.size() > hashTable.size() / 2 (:185-188, :282-311).
//   CellMetaDataNamesUsageCount         MemoryMapped::Vector<CellId>: the nodes that carry each name
//                                       (src/ExpressionMatrix.cpp:971-993).
#ifndef EM2_META_DATA_H
#define EM2_META_DATA_H

#include <stdint.h>

#include <string>
#include <vector>

namespace em2 {
namespace host {

constexpr uint32_t kInvalidStringId = 0xffffffffu;       // StringTable::invalidStringId

struct MetaDataNode {
    uint32_t nameId, valueId;
    uint64_t previous, next;
};
static_assert(sizeof(MetaDataNode) == 24, "VectorOfLists<pair<StringId, StringId>>::Node is 24 bytes");

class StringTable {
public:
    void create(uint64_t capacity);                        // createNew (:113-128): the next power of two
    void load(const std::string& prefix);                  // throws EM2_ERROR_IO for a table that cannot be used
    void write(const std::string& prefix) const;
    size_t size() const { return toc_.size() - 1u; }
    size_t capacity() const { return hash_.size(); }
    uint32_t find(const char* s, size_t length) const;     // operator() (:216-246)
    uint32_t find(const std::string& s) const { return find(s.data(), s.size()); }
    uint32_t insert(const std::string& s);                 // operator[] (:173-210)
    std::string get(uint32_t id) const;
private:
    bool holds(uint32_t id, const char* s, size_t length) const;
    void rehash();
    std::vector<uint32_t> toc_{0u};
    std::vector<char> data_;
    std::vector<uint32_t> hash_;
};

// The whole store in host memory: read when the directory is opened, written back by flush().
class MetaDataStore {
public:
    bool present = false;                                  // the directory has (or will have, once flushed) the files
    bool dirty = false;
    std::vector<uint64_t> toc, freeSlots;
    std::vector<MetaDataNode> nodes;
    StringTable names, values;
    std::vector<uint32_t> usage;

    // prefix: "Cell", or "Gene" for the gene meta data of a complete store (GeneMetaData.*, GeneMetaDataNames-*, ...), which has
    // the same containers (src/ExpressionMatrix.hpp) with one list per gene.
    void load(const std::string& directoryName, uint32_t cellCount, const std::string& prefix = "Cell");
    // One empty list per cell: what the reference's cellMetaData.push_back() per cell leaves (src/ExpressionMatrix.cpp:223).
    void create(uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity);
    void flush(const std::string& directoryName, const std::string& prefix = "Cell");
    // VectorOfLists::push_back() (:195-203): one more, empty list; its end node takes a free slot where there is one.
    void pushBackList();

    static constexpr uint64_t kNoNode = ~uint64_t(0);
    // The first node of the cell's list that carries nameId, kNoNode where there is none.  Every index is checked and the walk
    // ends after as many steps as there are nodes: a damaged store is EM2_ERROR_IO, not a loop or a wild read.
    uint64_t firstNode(uint32_t cell, uint32_t nameId) const;
    std::vector<uint64_t> list(uint32_t cell) const;       // the cell's nodes in list order
    void pushBack(uint32_t cell, uint32_t nameId, uint32_t valueId);      // insert(end(cell), ...) (:206-236)
    void erase(uint64_t node);                                            // (:247-261)
    void incrementUsage(uint32_t nameId);
    void decrementUsage(uint32_t nameId);
private:
    uint64_t allocateSlot();
    const MetaDataNode& at(uint64_t node) const;
    MetaDataNode& at(uint64_t node);
};

// The reference's new string tables start at 1 << 24 slots (the value table: a 64 MB file that it fills with 0xffffffff); a
// store created here starts at this and grows by the same doubling rule.  The reader takes the mask from the file's size.
constexpr uint64_t kNewStringTableCapacity = 1u << 12;

// histogramMetaData (src/ExpressionMatrix.cpp:1301-1323) of one or two fields over a cell set and their contingency table
// (:1369-1381) in the histograms' order.
struct MetaDataTable {
    std::vector<std::string> values[2];                    // count descending, then value ascending as std::string compares
    std::vector<uint64_t> counts[2];
    std::vector<uint64_t> row, column, count;              // the cells that are not zero, ascending by (row, column)
    std::vector<uint32_t> cellRow;                         // per cell of the set, in its order: the place of its value in values[0]
    uint64_t sums[4] = {0, 0, 0, 0};                       // sum v (v - 1) over the cells, t (t - 1) over rows, over columns; n
    int path = 0;                                          // of em2_contingency_sizes
};

// computeRandIndex (src/randIndex.hpp:58-97) from the three integer sums and n, expression by expression.  false where
// n (n - 1) >= 2^53: below that every partial sum of the reference's loops is an integer a double holds, so that the result is
// the reference's bit for bit in whatever order the table is summed.  n >= 1.
bool randIndexFromSums(uint64_t sumCells, uint64_t sumRows, uint64_t sumColumns, uint64_t n, double& randIndex, double& adjustedRandIndex);

void createMetaDataFiles(const std::string& directoryName, uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity);

}  // namespace host
}  // namespace em2

#endif
