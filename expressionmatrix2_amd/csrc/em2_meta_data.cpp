// em2_meta_data.cpp -- cell meta data: the store (em2_meta_data.h) and the ExpressionMatrix methods on it
// (src/ExpressionMatrix.cpp:880-1029, 1301-1390, 1560-1622), members of em2::host::Matrix.  Host code, except the contingency
// table of computeMetaDataRandIndex, which is em2_contingency_create (em2_contingency.hip) on one compact id per cell and field.
#include "em2_meta_data.h"
#include "em2_host.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <regex>

namespace em2 {
namespace host {

namespace {

[[noreturn]] void fail(int code, const std::string& message)
{
    Error e;
    e.code = code;
    e.message = message;
    throw e;
}

[[noreturn]] void damaged(const std::string& what) { fail(EM2_ERROR_IO, "The cell meta data store is damaged: " + what + "."); }

template <class T> void readVector(const std::string& path, std::vector<T>& out)
{
    MappedFile f;
    f.openExisting(path, false, sizeof(T));
    const T* p = static_cast<const T*>(f.data());
    out.assign(p, p + f.objectCount());
}

template <class T> void writeVector(const std::string& path, const std::vector<T>& in)
{
    MappedFile f;
    f.createNew(path, false, sizeof(T), in.size());
    if (!in.empty()) std::memcpy(f.data(), in.data(), in.size() * sizeof(T));
}

}  // namespace


// ---------------------------------------------------------------------------------------------------------
// StringTable
// ---------------------------------------------------------------------------------------------------------

void StringTable::create(uint64_t capacity)
{
    uint64_t n = 1;                                            // nextPowerOfTwoGreaterThanOrEqual (src/nextPowerOfTwo.hpp)
    while (n < capacity) n <<= 1;
    toc_.assign(1, 0u);
    data_.clear();
    hash_.assign(size_t(n), kInvalidStringId);
}

void StringTable::load(const std::string& prefix)
{
    readVector(prefix + "-strings.toc", toc_);
    readVector(prefix + "-strings.data", data_);
    readVector(prefix + "-hashTable", hash_);
    if (toc_.empty() || toc_[0] != 0u || toc_.back() != data_.size() || !std::is_sorted(toc_.begin(), toc_.end())) {
        damaged(prefix + "-strings is not a vector of strings");
    }
    if (hash_.empty() || (hash_.size() & (hash_.size() - 1u)) != 0u) damaged(prefix + "-hashTable is not a power of two long");
    size_t used = 0;
    for (const uint32_t id : hash_) {
        if (id == kInvalidStringId) continue;
        if (id >= size()) damaged(prefix + "-hashTable names a string that does not exist");
        used++;
    }
    // (a table without an empty slot would make the reference's look-up of an unknown string loop for ever)
    if (used != size() || used == hash_.size()) damaged(prefix + "-hashTable does not hold every string once");
}

void StringTable::write(const std::string& prefix) const
{
    writeVector(prefix + "-strings.toc", toc_);
    writeVector(prefix + "-strings.data", data_);
    writeVector(prefix + "-hashTable", hash_);
}

bool StringTable::holds(uint32_t id, const char* s, size_t length) const
{
    return toc_[id + 1u] - toc_[id] == length && (length == 0 || std::memcmp(data_.data() + toc_[id], s, length) == 0);
}

uint32_t StringTable::find(const char* s, size_t length) const
{
    if (hash_.empty()) return kInvalidStringId;
    const uint64_t mask = hash_.size() - 1u;
    uint64_t bucket = em2_murmur_hash_64a(s, int(length), 237) & mask;
    for (size_t probes = 0; probes < hash_.size(); probes++) {
        const uint32_t id = hash_[bucket];
        if (id == kInvalidStringId || holds(id, s, length)) return id;
        bucket = (bucket + 1u) & mask;
    }
    return kInvalidStringId;
}

uint32_t StringTable::insert(const std::string& s)
{
    if (s.size() > 0x7fffffffu) fail(EM2_ERROR_INVALID_ARGUMENT, "A meta data string is too long.");
    const uint64_t mask = hash_.size() - 1u;
    uint64_t bucket = em2_murmur_hash_64a(s.data(), int(s.size()), 237) & mask;
    while (true) {                                              // (load() and create() leave an empty slot, rehash keeps half)
        const uint32_t id = hash_[bucket];
        if (id == kInvalidStringId) break;
        if (holds(id, s.data(), s.size())) return id;
        bucket = (bucket + 1u) & mask;
    }
    if (size() >= kInvalidStringId - 1u || data_.size() + s.size() > 0xffffffffull) {
        fail(EM2_ERROR_UNSUPPORTED, "The meta data string table is full (32-bit string ids and offsets).");
    }
    const uint32_t id = uint32_t(size());
    hash_[bucket] = id;
    data_.insert(data_.end(), s.begin(), s.end());
    toc_.push_back(uint32_t(data_.size()));
    if (size() > hash_.size() / 2u) rehash();
    return id;
}

void StringTable::rehash()
{
    hash_.assign(2u * hash_.size(), kInvalidStringId);
    const uint64_t mask = hash_.size() - 1u;
    for (uint32_t id = 0; id < size(); id++) {
        uint64_t bucket = em2_murmur_hash_64a(data_.data() + toc_[id], int(toc_[id + 1u] - toc_[id]), 237) & mask;
        while (hash_[bucket] != kInvalidStringId) bucket = (bucket + 1u) & mask;
        hash_[bucket] = id;
    }
}

std::string StringTable::get(uint32_t id) const
{
    if (id >= size()) damaged("a node names a string that does not exist");
    return std::string(data_.data() + toc_[id], data_.data() + toc_[id + 1u]);
}


// ---------------------------------------------------------------------------------------------------------
// MetaDataStore
// ---------------------------------------------------------------------------------------------------------

void MetaDataStore::load(const std::string& directoryName, uint32_t cellCount, const std::string& prefix)
{
    const std::string base = directoryName + "/" + prefix + "MetaData";
    present = fileExists(base + ".toc");
    dirty = false;
    if (!present) return;
    readVector(base + ".toc", toc);
    readVector(base + ".data", nodes);
    readVector(base + ".freeSlots", freeSlots);
    readVector(base + "NamesUsageCount", usage);
    names.load(base + "Names");
    values.load(base + "Values");
    if (toc.size() != cellCount) {
        damaged(prefix + "MetaData holds " + std::to_string(toc.size()) + " lists for " + std::to_string(cellCount) + (prefix == "Cell" ? " cells" : " genes"));
    }
    if (usage.size() != names.size()) damaged(prefix + "MetaDataNamesUsageCount is not as long as the table of names");
}

void MetaDataStore::create(uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity)
{
    toc.resize(cellCount);
    nodes.assign(cellCount, MetaDataNode{0u, 0u, 0u, 0u});
    for (uint32_t cell = 0; cell < cellCount; cell++) {
        toc[cell] = cell;
        nodes[cell].previous = nodes[cell].next = cell;
    }
    freeSlots.clear();
    usage.clear();
    names.create(nameCapacity);
    values.create(valueCapacity);
    present = dirty = true;
}

void MetaDataStore::flush(const std::string& directoryName, const std::string& prefix)
{
    if (!present || !dirty) return;
    const std::string base = directoryName + "/" + prefix + "MetaData";
    writeVector(base + ".toc", toc);
    writeVector(base + ".data", nodes);
    writeVector(base + ".freeSlots", freeSlots);
    writeVector(base + "NamesUsageCount", usage);
    names.write(base + "Names");
    values.write(base + "Values");
    dirty = false;
}

void MetaDataStore::pushBackList()
{
    const uint64_t slot = allocateSlot();
    toc.push_back(slot);
    at(slot).previous = at(slot).next = slot;
    dirty = true;
}

const MetaDataNode& MetaDataStore::at(uint64_t node) const
{
    if (node >= nodes.size()) damaged("a list leaves the node store");
    return nodes[size_t(node)];
}

MetaDataNode& MetaDataStore::at(uint64_t node)
{
    if (node >= nodes.size()) damaged("a list leaves the node store");
    return nodes[size_t(node)];
}

uint64_t MetaDataStore::firstNode(uint32_t cell, uint32_t nameId) const
{
    const uint64_t end = toc[cell];
    uint64_t steps = 0;
    for (uint64_t node = at(end).next; node != end; node = at(node).next) {
        if (++steps > nodes.size()) damaged("a list does not come back to its end node");
        if (at(node).nameId == nameId) return node;
    }
    return kNoNode;
}

std::vector<uint64_t> MetaDataStore::list(uint32_t cell) const
{
    std::vector<uint64_t> result;
    const uint64_t end = toc[cell];
    for (uint64_t node = at(end).next; node != end; node = at(node).next) {
        if (result.size() >= nodes.size()) damaged("a list does not come back to its end node");
        result.push_back(node);
    }
    return result;
}

uint64_t MetaDataStore::allocateSlot()
{
    if (!freeSlots.empty()) {
        const uint64_t slot = freeSlots.back();
        if (slot >= nodes.size()) damaged("a free slot is outside the node store");
        freeSlots.pop_back();
        return slot;
    }
    nodes.push_back(MetaDataNode{0u, 0u, 0u, 0u});
    return nodes.size() - 1u;
}

void MetaDataStore::pushBack(uint32_t cell, uint32_t nameId, uint32_t valueId)
{
    const uint64_t end = toc[cell];
    const uint64_t previous = at(end).previous;
    at(previous);
    const uint64_t slot = allocateSlot();
    MetaDataNode& node = at(slot);
    node.nameId = nameId;
    node.valueId = valueId;
    at(previous).next = slot;
    node.previous = previous;
    at(end).previous = slot;
    node.next = end;
    dirty = true;
}

void MetaDataStore::erase(uint64_t node)
{
    const uint64_t previous = at(node).previous, next = at(node).next;
    at(previous);
    at(next);
    freeSlots.push_back(node);
    at(previous).next = next;
    at(next).previous = previous;
    dirty = true;
}

void MetaDataStore::incrementUsage(uint32_t nameId)
{
    if (usage.size() <= nameId) {
        if (usage.size() != nameId) damaged("CellMetaDataNamesUsageCount is not as long as the table of names");
        usage.push_back(1u);
    } else {
        ++usage[nameId];
    }
}

void MetaDataStore::decrementUsage(uint32_t nameId)
{
    if (nameId >= usage.size() || usage[nameId] == 0u) damaged("the usage count of a name that a node carries is zero");
    --usage[nameId];
}

void createMetaDataFiles(const std::string& directoryName, uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity)
{
    MetaDataStore store;
    store.create(cellCount, nameCapacity, valueCapacity);
    store.flush(directoryName);
}

bool randIndexFromSums(uint64_t sumCells, uint64_t sumRows, uint64_t sumColumns, uint64_t n, double& randIndex, double& adjustedRandIndex)
{
    if ((unsigned __int128)(n) * (n - 1u) >= (unsigned __int128)(1) << 53) return false;
    const double nDouble = double(n);
    const double nBinomial2 = 0.5 * nDouble * (nDouble - 1.);                 // :61
    double a = double(sumCells);                                               // :64-70: a sum of integers below 2^53
    a /= 2.;                                                                   // :71
    double b = -a;                                                             // :74
    b += 0.5 * double(sumRows);                                                // :75-78: every 0.5 * t * (t - 1.) is an integer
    double c = -a;                                                             // :81
    c += 0.5 * double(sumColumns);                                             // :82-85
    const double d = nBinomial2 - a - b - c;                                   // :88
    randIndex = (a + d) / (a + b + c + d);                                     // :91
    const double commonTerm = (a + b) * (a + c) + (c + d) * (b + d);           // :94
    const double adjustedRandIndexNumerator = nBinomial2 * (a + d) - commonTerm;
    const double adjustedRandIndexDenominator = nBinomial2 * nBinomial2 - commonTerm;
    adjustedRandIndex = adjustedRandIndexNumerator / adjustedRandIndexDenominator;
    return true;
}


// ---------------------------------------------------------------------------------------------------------
// Matrix
// ---------------------------------------------------------------------------------------------------------

void Matrix::openMetaData()
{
    std::unique_ptr<MetaDataStore> store(new MetaDataStore);
    store->load(directoryName_, cellCount());
    metaData_ = store.release();
}

void Matrix::closeMetaData()
{
    if (!metaData_) return;
    try {
        metaData_->flush(directoryName_);
    } catch (...) {                                            // (em2_matrix_flush reports what a destructor cannot)
    }
    delete metaData_;
    metaData_ = nullptr;
}

void Matrix::flush()
{
    metaData_->flush(directoryName_);
    flushIngest();
}

void Matrix::checkCellId(const char* who, uint32_t cellId) const
{
    if (cellId >= cellCount()) {
        fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": cell id " + std::to_string(cellId) + " is not below the cell count.");
    }
}

void Matrix::setCellMetaData(uint32_t cellId, const std::string& name, const std::string& value)
{
    checkCellId("setCellMetaData", cellId);
    MetaDataStore& store = *metaData_;
    if (!store.present) store.create(cellCount(), kNewStringTableCapacity, kNewStringTableCapacity);
    const uint32_t nameId = store.names.insert(name);                         // :944-945: the name first, both before the list
    const uint32_t valueId = store.values.insert(value);
    store.dirty = true;
    const uint64_t node = store.firstNode(cellId, nameId);
    if (node != MetaDataStore::kNoNode) {
        store.nodes[size_t(node)].valueId = valueId;                          // :957-962
        return;
    }
    store.pushBack(cellId, nameId, valueId);                                  // :965-966
    store.incrementUsage(nameId);
}

std::string Matrix::cellMetaDataValue(uint32_t cellId, const std::string& name) const
{
    checkCellId("getCellMetaDataValue", cellId);
    const MetaDataStore& store = *metaData_;
    if (!store.present) return "";
    const uint32_t nameId = store.names.find(name);
    if (nameId == kInvalidStringId) return "";                                // :884-887
    const uint64_t node = store.firstNode(cellId, nameId);
    if (node == MetaDataStore::kNoNode) return "";                            // :906
    const uint32_t valueId = store.nodes[size_t(node)].valueId;
    return valueId == kInvalidStringId ? "" : store.values.get(valueId);      // :897-901
}

std::vector<std::pair<std::string, std::string>> Matrix::cellMetaData(uint32_t cellId) const
{
    checkCellId("getCellMetaData", cellId);
    std::vector<std::pair<std::string, std::string>> result;
    const MetaDataStore& store = *metaData_;
    if (!store.present) return result;
    for (const uint64_t node : store.list(cellId)) {
        const MetaDataNode& n = store.nodes[size_t(node)];
        result.emplace_back(store.names.get(n.nameId), store.values.get(n.valueId));
    }
    return result;
}

const MappedFile& Matrix::cellSetForMetaData(const std::string& cellSetName) const
{
    const auto it = cellSets_.find(cellSetName);
    if (it == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " not found.");            // :1005, :1336
    return *it->second;
}

void Matrix::removeCellMetaData(const std::string& cellSetName, const std::string& metaDataName)
{
    const MappedFile& set = cellSetForMetaData(cellSetName);
    MetaDataStore& store = *metaData_;
    if (!store.present) return;
    const uint32_t nameId = store.names.find(metaDataName);
    if (nameId == kInvalidStringId) return;                                   // :1011-1015
    const uint32_t* cells = static_cast<const uint32_t*>(set.data());
    for (size_t i = 0; i < set.objectCount(); i++) {
        checkCellId("removeCellMetaData", cells[i]);
        const uint64_t node = store.firstNode(cells[i], nameId);
        if (node == MetaDataStore::kNoNode) continue;
        store.decrementUsage(nameId);                                         // :1022-1024
        store.erase(node);
    }
}

void Matrix::createCellSetUsingMetaData(const std::string& cellSetName, const std::string& metaDataFieldName, const std::string& matchString,
                                        bool useRegex)
{
    failIfCellSetExists(cellSetName);                                         // :1568-1570
    std::regex regex;
    if (useRegex) regex = matchString;                                        // :1573-1576 (std::regex_error for a bad expression)
    std::vector<uint32_t> cells;
    const MetaDataStore& store = *metaData_;
    const uint32_t nameId = store.present ? store.names.find(metaDataFieldName) : kInvalidStringId;
    if (nameId != kInvalidStringId) {
        // the verdict on a value, formed where the value is first met: 0 unknown, 1 in, 2 out
        std::vector<uint8_t> verdict(store.values.size(), uint8_t(0));
        for (uint32_t cellId = 0; cellId < cellCount(); cellId++) {           // :1584: ALL cells
            const uint64_t node = store.firstNode(cellId, nameId);
            if (node == MetaDataStore::kNoNode) continue;
            const uint32_t valueId = store.nodes[size_t(node)].valueId;
            if (valueId >= verdict.size()) store.values.get(valueId);         // (throws: damaged)
            if (verdict[valueId] == 0) {
                const std::string value = store.values.get(valueId);
                const bool in = useRegex ? std::regex_match(value.begin(), value.end(), regex) : value == matchString;   // :1598-1604
                verdict[valueId] = in ? 1 : 2;
            }
            if (verdict[valueId] == 1) cells.push_back(cellId);
        }
    }
    addCellSetOf(cellSetName, cells);                                         // :1621
}

namespace {

// raw[i] -> its rank among the distinct values of raw (ascending); returns how many there are.
uint32_t compactIds(const std::vector<uint32_t>& raw, std::vector<uint32_t>& compact, std::vector<uint32_t>& distinct)
{
    distinct = raw;
    std::sort(distinct.begin(), distinct.end());
    distinct.erase(std::unique(distinct.begin(), distinct.end()), distinct.end());
    compact.resize(raw.size());
    for (size_t i = 0; i < raw.size(); i++) {
        compact[i] = uint32_t(std::lower_bound(distinct.begin(), distinct.end(), raw[i]) - distinct.begin());
    }
    return uint32_t(distinct.size());
}

}  // namespace

void Matrix::metaDataTable(const std::string& cellSetName, const std::string& metaDataName0, const std::string* metaDataName1,
                           MetaDataTable& out) const
{
    out = MetaDataTable();
    const MappedFile& set = cellSetForMetaData(cellSetName);
    const MetaDataStore& store = *metaData_;
    const std::string* fieldNames[2] = {&metaDataName0, metaDataName1};
    const int fieldCount = metaDataName1 ? 2 : 1;
    uint32_t nameIds[2] = {kInvalidStringId, kInvalidStringId};
    for (int f = 0; f < fieldCount; f++) {                                    // :1341-1348
        nameIds[f] = store.present ? store.names.find(*fieldNames[f]) : kInvalidStringId;
        if (nameIds[f] == kInvalidStringId) fail(EM2_ERROR_RUNTIME, "Meta data field " + *fieldNames[f] + " not found.");
    }
    const size_t n = set.objectCount();
    if (n == 0) {
        // computeRandIndex's CZI_ASSERT(rowCount > 0) (src/randIndex.hpp:32): no cell, no histogram entry, no table row
        fail(EM2_ERROR_RUNTIME, "Assertion failed: rowCount > 0 (computeRandIndex: the cell set " + cellSetName + " is empty)");
    }

    // One id per cell and field.  The reference hands out "" both for a cell without the field and for a stored "": one id.
    const uint32_t storedEmpty = store.values.find("");
    const uint32_t* cells = static_cast<const uint32_t*>(set.data());
    std::vector<uint32_t> raw[2], compact[2], distinct[2];
    raw[0].resize(n);
    raw[1].assign(n, 0u);                                                     // (one field: a table of one column)
    for (size_t i = 0; i < n; i++) {
        checkCellId("computeMetaDataRandIndex", cells[i]);
        for (int f = 0; f < fieldCount; f++) {
            const uint64_t node = store.firstNode(cells[i], nameIds[f]);
            uint32_t valueId = node == MetaDataStore::kNoNode ? kInvalidStringId : store.nodes[size_t(node)].valueId;
            if (valueId == kInvalidStringId) valueId = storedEmpty;
            else if (valueId >= store.values.size()) store.values.get(valueId);           // (throws: damaged)
            raw[f][i] = valueId;
        }
    }
    const uint32_t n0 = compactIds(raw[0], compact[0], distinct[0]);
    const uint32_t n1 = compactIds(raw[1], compact[1], distinct[1]);

    em2_contingency* table = nullptr;
    const int status = em2_contingency_create(compact[0].data(), compact[1].data(), n, n0, n1, 0, &table);
    if (status != EM2_OK) fail(status, em2_last_error());
    std::unique_ptr<em2_contingency, void (*)(em2_contingency*)> owner(table, em2_contingency_free);
    uint64_t nonZeroCount = 0;
    em2_contingency_sizes(table, nullptr, nullptr, nullptr, &nonZeroCount, &out.path);
    std::vector<uint64_t> totals[2] = {std::vector<uint64_t>(n0), std::vector<uint64_t>(n1)};
    std::vector<uint32_t> i0(nonZeroCount), i1(nonZeroCount);
    std::vector<uint64_t> count(nonZeroCount);
    em2_contingency_get(table, totals[0].data(), totals[1].data(), i0.data(), i1.data(), count.data(), out.sums);
    out.sums[3] = n;

    // The histograms' order (:1322, OrderPairsBySecondGreaterThenByFirstLess): the strings are touched here only.
    std::vector<uint32_t> position[2];
    for (int f = 0; f < fieldCount; f++) {
        const size_t valueCount = distinct[f].size();
        std::vector<std::string> strings(valueCount);
        for (size_t v = 0; v < valueCount; v++) strings[v] = distinct[f][v] == kInvalidStringId ? std::string() : store.values.get(distinct[f][v]);
        std::vector<uint32_t> order(valueCount);
        for (size_t v = 0; v < valueCount; v++) order[v] = uint32_t(v);
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            if (totals[f][x] != totals[f][y]) return totals[f][x] > totals[f][y];
            return strings[x] < strings[y];
        });
        position[f].resize(valueCount);
        for (size_t rank = 0; rank < valueCount; rank++) {
            position[f][order[rank]] = uint32_t(rank);
            out.values[f].push_back(strings[order[rank]]);
            out.counts[f].push_back(totals[f][order[rank]]);
        }
    }
    out.cellRow.resize(n);
    for (size_t i = 0; i < n; i++) out.cellRow[i] = position[0][compact[0][i]];
    if (fieldCount == 2) {
        std::vector<size_t> order(nonZeroCount);
        for (size_t t = 0; t < nonZeroCount; t++) order[t] = t;
        std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
            const uint32_t rx = position[0][i0[x]], ry = position[0][i0[y]];
            return rx != ry ? rx < ry : position[1][i1[x]] < position[1][i1[y]];
        });
        for (const size_t t : order) {
            out.row.push_back(position[0][i0[t]]);
            out.column.push_back(position[1][i1[t]]);
            out.count.push_back(count[t]);
        }
    }
}

void Matrix::computeMetaDataRandIndex(const std::string& cellSetName, const std::string& metaDataName0, const std::string& metaDataName1,
                                      double& randIndex, double& adjustedRandIndex) const
{
    MetaDataTable table;
    metaDataTable(cellSetName, metaDataName0, &metaDataName1, table);
    if (!randIndexFromSums(table.sums[0], table.sums[1], table.sums[2], table.sums[3], randIndex, adjustedRandIndex)) {
        fail(EM2_ERROR_UNSUPPORTED, "computeMetaDataRandIndex: with " + std::to_string(table.sums[3]) + " cells n (n - 1) is not below 2^53, "
                                    "where the reference's sums of doubles stop being exact; at most 94906266 cells are supported.");
    }
}

}  // namespace host
}  // namespace em2
