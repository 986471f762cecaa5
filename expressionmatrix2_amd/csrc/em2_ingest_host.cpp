// em2_ingest_host.cpp -- ingest on the host: a new, complete store (ExpressionMatrix::createNew), addGene, the name look-ups,
// addCell, and the driver of the bulk add, whose per-cell work (zeros out, gene map, sums, sort, duplicate check, Cell record)
// is the device pass of em2_ingest.hip.  Members of em2::host::Matrix.
#include "em2_ingest.h"

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <memory>
#include <unordered_map>
#include <unordered_set>

#include <sys/stat.h>
#include <unistd.h>

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

const uint32_t kInvalidId = 0xffffffffu;                  // invalidGeneId, invalidCellId (src/Ids.hpp)
const uint64_t kDefaultChunkBytes = uint64_t(1) << 30;
const char* const kNoWriteAccess = "write access";        // IngestState::missing of a complete store that cannot be written

// The directory has the files of a complete store: the name look-ups work, whether or not it can be written.
bool hasNames(const IngestState& s) { return s.missing.empty() || s.missing == kNoWriteAccess; }

[[noreturn]] void failMissing(const char* who, const std::string& directoryName, const IngestState& s)
{
    fail(EM2_ERROR_RUNTIME, std::string(who) + ": " + directoryName + " has no " + s.missing +
                                " (gene and cell names and ingest need a store that ExpressionMatrix.create made)");
}

const IngestState& namesOf(const IngestState* s, const std::string& directoryName, const char* who)
{
    if (!hasNames(*s)) failMissing(who, directoryName, *s);
    return *s;
}

}  // namespace


int storeCell(std::vector<em2_count>& entries, CellRecord& cell, uint32_t& duplicateGene)
{
    std::memset(&cell, 0, sizeof(cell));
    duplicateGene = kInvalidId;
    size_t kept = 0;
    for (const em2_count& e : entries) {                                      // :245-260
        const float value = e.count;
        if (value < 0.f) return kIngestNegative;
        if (value == 0.f) continue;
        cell.sum1 += value;
        cell.sum2 += value * value;                                           // a float product
        entries[kept++] = e;
    }
    entries.resize(kept);
    cell.norm2 = std::sqrt(cell.sum2);                                        // :261-263
    cell.norm1Inverse = 1. / cell.sum1;
    cell.norm2Inverse = 1. / cell.norm2;
    std::sort(entries.begin(), entries.end(), [](const em2_count& x, const em2_count& y) { return x.gene < y.gene; });       // :266-267
    for (size_t i = 1; i < entries.size(); i++) {                             // :272-277
        if (entries[i - 1].gene == entries[i].gene) {
            duplicateGene = entries[i].gene;
            return kIngestDuplicate;
        }
    }
    return kIngestOk;
}


Matrix* Matrix::create(const std::string& directoryName)
{
    if (fileExists(directoryName)) fail(EM2_ERROR_RUNTIME, "Directory " + directoryName + " already exists.");
    if (::mkdir(directoryName.c_str(), 0777) == -1) {
        fail(EM2_ERROR_IO, "Cannot create directory " + directoryName + ": " + std::string(strerror(errno)));
    }
    const std::string d = directoryName + "/";
    {
        StringTable names;
        names.create(kNewStringTableCapacity);
        names.write(d + "GeneNames");                                         // :72
        names.write(d + "CellNames");                                         // :80
        MetaDataStore store;
        store.create(0, kNewStringTableCapacity, kNewStringTableCapacity);
        store.flush(directoryName, "Gene");                                   // :73-76
        store.dirty = true;
        store.flush(directoryName, "Cell");                                   // :81-84
        MappedFile f;
        f.createNew(d + "Cells", false, sizeof(CellRecord), 0);               // :79
        f.createNew(d + "CellExpressionCounts.toc", false, sizeof(uint64_t), 1);          // :85: the single 0
        f.createNew(d + "CellExpressionCounts.data", false, sizeof(em2_count), 0);
        f.createNew(d + "CellSet-AllCells", false, sizeof(uint32_t), 0);      // :88-90
        f.createNew(d + "GeneSet-AllGenes-GlobalIds", false, sizeof(uint32_t), 0);        // :93
        f.createNew(d + "GeneSet-AllGenes-LocalIds", false, sizeof(uint32_t), 0);
    }
    return new Matrix(directoryName);
}

void Matrix::openIngest(bool writable)
{
    std::unique_ptr<IngestState> s(new IngestState);
    const std::string d = directoryName_ + "/";
    for (const char* name : {"GeneNames-strings.toc", "GeneMetaData.toc", "Cells", "CellNames-strings.toc", "CellMetaData.toc"}) {
        if (!fileExists(d + name)) {
            s->missing = name;
            break;
        }
    }
    if (s->missing.empty()) {
        writable = writable && ::access(directoryName_.c_str(), W_OK) == 0;
        s->geneNames.load(d + "GeneNames");
        s->cellNames.load(d + "CellNames");
        s->geneMetaData.load(directoryName_, uint32_t(s->geneNames.size()), "Gene");
        s->cells.openExisting(d + "Cells", false, sizeof(CellRecord), writable);
        GeneSet& allGenes = *geneSets_["AllGenes"];
        MappedFile& allCells = *cellSets_["AllCells"];
        // the sanity checks of accessExisting (:146-151)
        if (s->cellNames.size() != cellCount() || s->cells.objectCount() != cellCount() || allCells.objectCount() != cellCount() ||
            allGenes.size() != s->geneNames.size()) {
            fail(EM2_ERROR_IO, "The store " + directoryName_ + " is damaged: CellNames, Cells, CellExpressionCounts, AllCells or "
                               "GeneNames and AllGenes do not agree in size.");
        }
        if (writable) {
            toc_.openExisting(d + "CellExpressionCounts.toc", false, sizeof(uint64_t), true);
            data_.openExisting(d + "CellExpressionCounts.data", false, sizeof(em2_count), true);
            allCells.openExisting(d + "CellSet-AllCells", false, sizeof(uint32_t), true);
            allGenes.globalIds.openExisting(d + "GeneSet-AllGenes-GlobalIds", false, sizeof(uint32_t), true);
            allGenes.localIds.openExisting(d + "GeneSet-AllGenes-LocalIds", false, sizeof(uint32_t), true);
        } else {
            s->missing = kNoWriteAccess;
        }
    }
    ingest_ = s.release();
}

void Matrix::flushIngest()
{
    if (!ingest_ || !ingest_->missing.empty()) return;
    ingest_->geneMetaData.flush(directoryName_, "Gene");
    if (ingest_->dirty) {
        ingest_->geneNames.write(directoryName_ + "/GeneNames");
        ingest_->cellNames.write(directoryName_ + "/CellNames");
        ingest_->dirty = false;
    }
}

void Matrix::closeIngest()
{
    if (!ingest_) return;
    try {
        flushIngest();
    } catch (...) {                                            // (em2_matrix_flush reports what a destructor cannot)
    }
    delete ingest_;
    ingest_ = nullptr;
}

IngestState& Matrix::ingest(const char* who) const
{
    if (!ingest_->missing.empty()) failMissing(who, directoryName_, *ingest_);
    return *ingest_;
}

uint32_t Matrix::geneCount() const
{
    return hasNames(*ingest_) ? uint32_t(ingest_->geneNames.size()) : uint32_t(geneSet("AllGenes").localIds.objectCount());
}

std::string Matrix::geneName(uint32_t geneId) const
{
    const IngestState& s = namesOf(ingest_, directoryName_, "geneName");
    if (geneId >= s.geneNames.size()) {
        fail(EM2_ERROR_INVALID_ARGUMENT, "geneName: gene id " + std::to_string(geneId) + " is not below the gene count.");
    }
    return s.geneNames.get(geneId);
}

uint32_t Matrix::geneIdFromName(const std::string& geneName) const
{
    return namesOf(ingest_, directoryName_, "geneIdFromName").geneNames.find(geneName);
}

uint32_t Matrix::cellIdFromString(const std::string& s) const
{
    const IngestState& state = namesOf(ingest_, directoryName_, "cellIdFromString");
    // lexical_cast<CellId> (:826): the whole text is an unsigned decimal number that a CellId holds.  Accepted here: an
    // optional '+', then digits only, value at most 0xffffffff -- no blanks, no '-', no hexadecimal.
    size_t at = !s.empty() && s[0] == '+' ? 1 : 0;
    if (at < s.size() && s.size() - at <= 10) {
        uint64_t value = 0;
        bool digits = true;
        for (; at < s.size(); at++) {
            if (s[at] < '0' || s[at] > '9') {
                digits = false;
                break;
            }
            value = 10u * value + uint64_t(s[at] - '0');
        }
        if (digits && value < cellCount()) return uint32_t(value);            // :827-829
    }
    return state.cellNames.find(s);                                           // :835
}

bool Matrix::addGene(const std::string& geneName)
{
    IngestState& s = ingest("addGene");
    if (s.geneNames.find(geneName) != kInvalidStringId) return false;
    const uint32_t geneId = s.geneNames.insert(geneName);                     // :20
    s.dirty = true;
    MetaDataStore& store = s.geneMetaData;
    store.pushBackList();                                                     // :23
    const uint32_t nameId = store.names.insert("GeneName");                   // :26, setGeneMetaData :53-58: no such field yet
    const uint32_t valueId = store.values.insert(geneName);
    store.pushBack(geneId, nameId, valueId);
    store.incrementUsage(nameId);
    GeneSet& all = *geneSets_["AllGenes"];                                    // GeneSet::addGene (src/GeneSet.cpp:52-62)
    const size_t oldSize = all.localIds.objectCount();
    if (geneId >= oldSize) {
        all.localIds.resize(size_t(geneId) + 1u);
        uint32_t* local = static_cast<uint32_t*>(all.localIds.data());
        for (size_t i = oldSize; i <= geneId; i++) local[i] = kInvalidId;
    }
    static_cast<uint32_t*>(all.localIds.data())[geneId] = all.size();
    all.globalIds.append(&geneId, 1);
    return true;
}

void Matrix::commitCell(const std::vector<std::pair<std::string, std::string>>& metaData, const em2_count* entries, uint64_t entryCount,
                        const void* cellRecord)
{
    IngestState& s = *ingest_;
    const uint32_t cellId = s.cellNames.insert(metaData.front().second);      // :218
    s.dirty = true;
    MetaDataStore& store = *metaData_;
    store.pushBackList();                                                     // :223-237
    for (const auto& p : metaData) {
        const uint32_t nameId = store.names.insert(p.first);
        store.incrementUsage(nameId);
        const uint32_t valueId = store.values.insert(p.second);
        store.pushBack(cellId, nameId, valueId);
    }
    data_.append(entries, entryCount);                                        // :244-267
    const uint64_t end = data_.objectCount();
    toc_.append(&end, 1);
    cellSets_["AllCells"]->append(&cellId, 1);                                // :280
    s.cells.append(cellRecord, 1);                                            // :283
}

uint32_t Matrix::writeCells(const std::vector<std::string>& newGenes, size_t cellCount,
                            const std::function<const std::vector<std::pair<std::string, std::string>>*(size_t)>& metaDataOf,
                            const uint64_t* toc, const em2_count* data, const void* cellRecords)
{
    for (const std::string& name : newGenes) addGene(name);
    uint32_t added = 0;
    for (size_t i = 0; i < cellCount; i++) {
        const std::vector<std::pair<std::string, std::string>>* metaData = metaDataOf(i);
        if (!metaData) continue;
        commitCell(*metaData, data + toc[i], toc[i + 1u] - toc[i], static_cast<const CellRecord*>(cellRecords) + i);
        added++;
    }
    return added;
}

uint32_t Matrix::addCell(const std::vector<std::pair<std::string, std::string>>& metaDataArgument,
                         const std::vector<std::pair<std::string, float>>& expressionCounts)
{
    IngestState& s = ingest("addCell");
    std::vector<std::pair<std::string, std::string>> metaData = metaDataArgument;
    bool cellNameWasFound = false;
    for (auto& p : metaData) {                                                // :190-204
        if (p.first == "CellName") {
            cellNameWasFound = true;
            std::swap(p, metaData.front());
            break;
        }
    }
    if (!cellNameWasFound) fail(EM2_ERROR_RUNTIME, "CellName missing from cell meta data.");
    const std::string& cellName = metaData.front().second;
    if (s.cellNames.find(cellName) != kInvalidStringId) fail(EM2_ERROR_RUNTIME, "Cell name " + cellName + " already exists.");
    if (cellCount() >= kInvalidId - 1u) fail(EM2_ERROR_UNSUPPORTED, "addCell: the store is full (32-bit cell ids).");

    // Check first, then write: the ids the genes will get, in the order they are met (:246-248).
    std::vector<std::string> newGenes;
    std::unordered_map<std::string, uint32_t> newGeneIds;
    std::vector<em2_count> entries;
    entries.reserve(expressionCounts.size());
    for (const auto& p : expressionCounts) {
        uint32_t geneId = s.geneNames.find(p.first);
        if (geneId == kInvalidStringId) {
            const auto it = newGeneIds.find(p.first);
            if (it != newGeneIds.end()) {
                geneId = it->second;
            } else {
                geneId = uint32_t(s.geneNames.size() + newGenes.size());
                newGeneIds.emplace(p.first, geneId);
                newGenes.push_back(p.first);
            }
        }
        em2_count e;
        e.gene = geneId;
        e.count = p.second;
        entries.push_back(e);
    }
    CellRecord cell;
    uint32_t duplicateGene = kInvalidId;
    const int status = storeCell(entries, cell, duplicateGene);
    if (status == kIngestNegative) fail(EM2_ERROR_RUNTIME, "Negative expression count encountered.");
    if (status == kIngestDuplicate) {
        const std::string duplicateGeneName = duplicateGene < s.geneNames.size() ? s.geneNames.get(duplicateGene)
                                                                                  : newGenes[duplicateGene - s.geneNames.size()];
        fail(EM2_ERROR_RUNTIME, "Duplicate expression count for cell " + cellName + " gene " + duplicateGeneName);
    }
    for (const std::string& name : newGenes) addGene(name);
    const uint32_t cellId = cellCount();
    commitCell(metaData, entries.data(), entries.size(), &cell);
    return cellId;
}

void Matrix::addCellsFromCsr(const std::vector<std::string>& geneNames, const std::vector<std::string>& cellNames, const uint64_t* indptr,
                             const uint32_t* indices, const float* values, uint64_t entryCount, const uint8_t* skip,
                             const std::string& cellNamePrefix, const std::vector<std::pair<std::string, std::string>>& cellMetaData,
                             uint64_t chunkBytes, uint32_t& firstCellId, uint32_t& addedCellCount)
{
    const char* who = "addCellsFromCsr";
    IngestState& s = ingest(who);
    const size_t barcodeCount = cellNames.size();
    // The reference asserts these (src/ExpressionMatrixHdf5.cpp:158-171); here they are refused before any work.
    if (barcodeCount >= kInvalidId || geneNames.size() >= kInvalidId) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": too many names");
    if (indptr[0] != 0) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": indptr does not start at 0");
    for (size_t i = 0; i < barcodeCount; i++) {
        if (indptr[i + 1] < indptr[i]) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": indptr descends");
        if (indptr[i + 1] - indptr[i] >= (uint64_t(1) << 31)) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a row has 2^31 entries or more");
    }
    if (indptr[barcodeCount] != entryCount) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": indptr does not end at the length of indices and data");
    for (uint64_t j = 0; j < entryCount; j++) {
        if (indices[j] >= geneNames.size()) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": an index is not below the number of gene names");
    }
    {                                                                         // :72-90
        std::vector<std::string> sorted = geneNames;
        std::sort(sorted.begin(), sorted.end());
        for (size_t i = 1; i < sorted.size(); i++) {
            if (sorted[i - 1] == sorted[i]) fail(EM2_ERROR_RUNTIME, "Duplicate gene name " + sorted[i] + " in geneNames");
        }
    }

    // The gene ids after the addGene of every name in order (:116-118), without adding one yet.
    std::vector<uint32_t> geneIdOfIndex(geneNames.size());
    std::vector<std::string> newGenes;
    for (size_t i = 0; i < geneNames.size(); i++) {
        uint32_t geneId = s.geneNames.find(geneNames[i]);
        if (geneId == kInvalidStringId) {
            geneId = uint32_t(s.geneNames.size() + newGenes.size());
            newGenes.push_back(geneNames[i]);
        }
        geneIdOfIndex[i] = geneId;
    }
    if (s.geneNames.size() + newGenes.size() >= kInvalidId) fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": the store is full (32-bit gene ids).");

    // The device pass, chunk by chunk of barcodes, and the checks in barcode order; nothing is written before the last one.
    if (chunkBytes == 0) chunkBytes = kDefaultChunkBytes;
    std::vector<uint64_t> allToc(1, 0u);                                      // per barcode, skipped ones of length 0
    std::vector<em2_count> allData;
    std::vector<CellRecord> allCells(barcodeCount);
    std::unordered_set<std::string> namesOfBatch;
    uint64_t kept = 0;
    for (size_t i = 0; i < barcodeCount; i++) kept += skip && skip[i] ? 0u : 1u;
    if (uint64_t(cellCount()) + kept >= kInvalidId - 1u) fail(EM2_ERROR_UNSUPPORTED, std::string(who) + ": the store is full (32-bit cell ids).");
    std::vector<uint64_t> chunkIndptr;
    std::vector<uint8_t> chunkSkip;
    std::vector<uint32_t> keptCount, status, duplicateGene;
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    std::vector<CellRecord> cells;
    for (size_t begin = 0; begin < barcodeCount && kept;) {
        size_t end = begin + 1;
        const auto bytesOf = [&](size_t e) { return (indptr[e] - indptr[begin]) * 16u + uint64_t(e - begin) * 96u; };
        while (end < barcodeCount && bytesOf(end + 1) <= chunkBytes) end++;
        const uint32_t n = uint32_t(end - begin);
        chunkIndptr.resize(size_t(n) + 1u);
        chunkSkip.resize(n);
        for (uint32_t i = 0; i <= n; i++) chunkIndptr[i] = indptr[begin + i] - indptr[begin];
        for (uint32_t i = 0; i < n; i++) chunkSkip[i] = skip && skip[begin + i] ? 1 : 0;
        bool failed = false;
        const int rc = ingestChunkOnDevice(chunkIndptr.data(), indices + indptr[begin], values + indptr[begin], chunkSkip.data(), n,
                                           geneIdOfIndex.data(), uint32_t(geneIdOfIndex.size()), keptCount, status, duplicateGene, toc,
                                           data, cells, &failed);
        if (rc != EM2_OK) fail(rc, em2_last_error());
        for (uint32_t i = 0; i < n; i++) {                                    // addCell's order within a barcode: name, negative, duplicate
            if (chunkSkip[i]) continue;                                       // :177-179: neither named nor checked
            const std::string cellName = cellNamePrefix + "-" + cellNames[begin + i];             // :166
            if (s.cellNames.find(cellName) != kInvalidStringId || !namesOfBatch.insert(cellName).second) {
                fail(EM2_ERROR_RUNTIME, "Cell name " + cellName + " already exists.");
            }
            if (status[i] == kIngestNegative) fail(EM2_ERROR_RUNTIME, "Negative expression count encountered.");
            if (status[i] == kIngestDuplicate) {
                const uint32_t g = duplicateGene[i];
                const std::string duplicateGeneName = g < s.geneNames.size() ? s.geneNames.get(g) : newGenes[g - s.geneNames.size()];
                fail(EM2_ERROR_RUNTIME, "Duplicate expression count for cell " + cellName + " gene " + duplicateGeneName);
            }
            if (status[i] != kIngestOk) fail(EM2_ERROR_RUNTIME, std::string(who) + ": the device pass reports an index out of range");
        }
        if (failed) fail(EM2_ERROR_RUNTIME, std::string(who) + ": the device pass reports an error in a skipped barcode");
        const uint64_t base = allData.size();
        allData.insert(allData.end(), data.begin(), data.end());
        for (uint32_t i = 0; i < n; i++) {
            allToc.push_back(base + toc[i + 1u]);
            allCells[begin + i] = cells[i];
        }
        begin = end;
    }
    if (!kept) allToc.assign(barcodeCount + 1u, 0u);

    // Write (:116-118, then addCell per barcode): string-table ids come out in the order of first insertion.
    firstCellId = cellCount();
    std::vector<std::pair<std::string, std::string>> metaData(cellMetaData.size() + 1u);          // :122-124
    metaData.front().first = "CellName";
    std::copy(cellMetaData.begin(), cellMetaData.end(), metaData.begin() + 1);
    addedCellCount = writeCells(newGenes, barcodeCount,
                                [&](size_t i) -> const std::vector<std::pair<std::string, std::string>>* {
                                    if (skip && skip[i]) return nullptr;
                                    metaData.front().second = cellNamePrefix + "-" + cellNames[i];
                                    return &metaData;
                                },
                                allToc.data(), allData.data(), allCells.data());
}

}  // namespace host
}  // namespace em2
