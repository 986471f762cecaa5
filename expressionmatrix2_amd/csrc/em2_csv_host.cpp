// em2_csv_host.cpp -- the host side of addCells and addCellMetaData: the reference's tokenizer and getline restated (there is
// no Boost to link), the cell meta data file, the header rules, the order of the checks and the error texts of
// src/ExpressionMatrix.cpp:380-654, and the host path of the expression counts file.  The device path (em2_csv.hip) replaces
// only the per-line work of :559-626; every line it hands back (a line with an escape, a field it cannot prove) comes here.
#include "em2_csv.h"

#include <cerrno>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <set>
#include <unordered_set>

#include <fcntl.h>
#include <sys/mman.h>
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

[[noreturn]] void failRuntime(const std::string& message) { fail(EM2_ERROR_RUNTIME, message); }

const uint32_t kNone = 0xffffffffu;
const uint64_t kDefaultCsvChunkBytes = uint64_t(256) << 20;
const uint64_t kMaxCsvChunkBytes = 0xf0000000u;            // the device's offsets are 32-bit

bool isBlank(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

// A whole file, read-only.  ok == false: it could not be opened.
struct MappedText {
    const char* p = "";
    size_t bytes = 0;
    void* base = nullptr;
    bool ok = false;
    explicit MappedText(const std::string& path)
    {
        const int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) return;
        struct stat st;
        if (::fstat(fd, &st) == 0 && S_ISREG(st.st_mode)) {
            ok = true;
            bytes = size_t(st.st_size);
            if (bytes) {
                base = ::mmap(nullptr, bytes, PROT_READ, MAP_PRIVATE, fd, 0);
                if (base == MAP_FAILED) {
                    base = nullptr;
                    ok = false;
                } else {
                    p = static_cast<const char*>(base);
                }
            }
        }
        ::close(fd);
    }
    ~MappedText()
    {
        if (base) ::munmap(base, bytes);
    }
    MappedText(const MappedText&) = delete;
    MappedText& operator=(const MappedText&) = delete;
};

void stripCr(const char* line, size_t& length)
{
    if (length && line[length - 1] == 13) length--;
}

// countTokensInSecondLine (src/tokenize.cpp:140-173).  Departure: an empty second line is an error (the reference reads
// line[-1]).
size_t countTokensInSecondLine(const MappedText& file, const std::string& fileName, const std::string& separators, const char* what)
{
    if (!file.ok) failRuntime("Could not open file " + fileName);
    LineReader reader(file.p, file.bytes);
    const char* line;
    size_t length;
    if (!reader.next(line, length)) failRuntime("Error reading header line of file " + fileName);
    if (!reader.next(line, length)) failRuntime("Error reading the second line of file " + fileName);
    if (length == 0) failRuntime(std::string("Empty line in ") + what + " file " + fileName);
    stripCr(line, length);
    std::vector<std::string> tokens;
    tokenize(separators, line, length, tokens, false);
    return tokens.size();
}

// The count of a trimmed token (:611-624).  0: skipped ("0", "0."); 1: *value is set; 2: strtof consumed nothing.
int countOf(const std::string& token, float* value)
{
    if (token == "0" || token == "0.") return 0;
    const char* begin = token.c_str();
    char* check = nullptr;
    *value = std::strtof(begin, &check);
    return check == begin ? 2 : 1;
}

struct HostLine {
    uint64_t begin, end, firstBegin, firstEnd;             // offsets into the body; [begin, end) without '\n' and one '\r'
    uint32_t tokenCount, status;
};

}  // namespace


void tokenize(const std::string& separators, const char* line, size_t length, std::vector<std::string>& tokens, bool trim)
{
    tokens.clear();
    if (length == 0) return;
    const auto isSeparator = [&](char c) { return separators.find(c) != std::string::npos; };
    bool inQuote = false;
    std::string token;
    for (size_t i = 0; i < length; i++) {
        const char c = line[i];
        if (c == '\\') {
            if (++i == length) failRuntime("cannot end with escape");
            const char n = line[i];
            if (n == 'n') token += '\n';
            else if (n == '"' || n == '\\' || isSeparator(n)) token += n;
            else failRuntime("unknown escape sequence");
        } else if (isSeparator(c) && !inQuote) {
            tokens.push_back(token);
            token.clear();
        } else if (c == '"') {
            inQuote = !inQuote;
        } else {
            token += c;
        }
    }
    tokens.push_back(token);
    if (trim) {
        for (std::string& t : tokens) {
            size_t b = 0, e = t.size();
            while (b < e && isBlank(t[b])) b++;
            while (e > b && isBlank(t[e - 1])) e--;
            t = t.substr(b, e - b);
        }
    }
}

bool LineReader::next(const char*& line, size_t& length)
{
    if (at == end) return false;
    line = at;
    const void* newline = std::memchr(at, '\n', size_t(end - at));
    if (newline) {
        length = size_t(static_cast<const char*>(newline) - at);
        at = static_cast<const char*>(newline) + 1;
    } else {
        length = size_t(end - at);
        at = end;
    }
    return true;
}

bool csvSeparatorsRunOnDevice(const std::string& separators)
{
    if (separators.empty() || separators.size() > 8) return false;
    for (char c : separators) {
        if (c == '"' || c == '\\' || c == '\n' || c == '\r' || c == 0) return false;
    }
    return true;
}

void Matrix::addCellsFromCsv(const std::string& expressionCountsFileName, const std::string& expressionCountsFileSeparators,
                             const std::string& cellMetaDataFileName, const std::string& cellMetaDataFileSeparators,
                             const std::vector<std::pair<std::string, std::string>>& additionalCellMetaData, uint64_t chunkBytes,
                             bool useDevice, uint32_t& firstCellId, uint32_t& addedCellCount, uint64_t* deferredFieldCount)
{
    typedef std::vector<std::pair<std::string, std::string>> MetaData;
    IngestState& s = ingest("addCells");
    if (deferredFieldCount) *deferredFieldCount = 0;
    const char* line;
    size_t length;
    std::vector<std::string> tokens;

    // The cell meta data file (:393-488).
    const MappedText metaDataFile(cellMetaDataFileName);
    const size_t metaDataCount = countTokensInSecondLine(metaDataFile, cellMetaDataFileName, cellMetaDataFileSeparators, "cell meta data");
    LineReader metaDataReader(metaDataFile.p, metaDataFile.bytes);
    metaDataReader.next(line, length);
    if (length == 0) failRuntime("Error reading header line from cell meta data file " + cellMetaDataFileName);
    stripCr(line, length);
    tokenize(cellMetaDataFileSeparators, line, length, tokens, false);
    std::vector<std::string> metaDataNames(1, "CellName");
    if (tokens.size() == metaDataCount) {
        metaDataNames.insert(metaDataNames.end(), tokens.begin() + 1, tokens.end());
    } else if (tokens.size() == metaDataCount - 1) {
        metaDataNames.insert(metaDataNames.end(), tokens.begin(), tokens.end());
    } else {
        failRuntime("Number of tokens in header line of cell meta data file " + cellMetaDataFileName + " is inconsistent with file contents.");
    }
    std::vector<std::vector<std::string>> metaDataInFile;
    std::map<std::string, uint32_t> metaDataInFileMap;
    while (metaDataReader.next(line, length)) {
        if (length == 0) failRuntime("Empty line in cell meta data file " + cellMetaDataFileName);
        stripCr(line, length);
        tokenize(cellMetaDataFileSeparators, line, length, tokens, false);
        if (tokens.size() != metaDataNames.size()) {
            failRuntime("Unexpected number of items in line of cell meta data file " + cellMetaDataFileName);
        }
        const std::string& cellName = tokens[0];
        if (metaDataInFileMap.find(cellName) != metaDataInFileMap.end()) {
            failRuntime("Duplicate cell name " + cellName + " in cell meta data file " + cellMetaDataFileName);
        }
        metaDataInFileMap.insert(std::make_pair(cellName, uint32_t(metaDataInFile.size())));
        metaDataInFile.push_back(tokens);
    }

    // The header of the expression counts file and the cells to keep (:492-543), in the order of the file's columns.
    const MappedText expressionFile(expressionCountsFileName);
    const size_t expectedTokenCount =
        countTokensInSecondLine(expressionFile, expressionCountsFileName, expressionCountsFileSeparators, "expression counts");
    const size_t cellCountInExpressionFile = expectedTokenCount - 1;
    if (expectedTokenCount >= kNone) fail(EM2_ERROR_UNSUPPORTED, "addCells: too many columns in " + expressionCountsFileName);
    LineReader expressionReader(expressionFile.p, expressionFile.bytes);
    expressionReader.next(line, length);
    if (length == 0) failRuntime("Error reading header line from expression counts file " + expressionCountsFileName);
    stripCr(line, length);
    tokenize(expressionCountsFileSeparators, line, length, tokens, true);
    std::vector<std::string> cellNamesInExpressionCountsFile;
    if (tokens.size() == cellCountInExpressionFile) {
        cellNamesInExpressionCountsFile = tokens;
    } else if (tokens.size() == cellCountInExpressionFile + 1) {
        cellNamesInExpressionCountsFile.assign(tokens.begin() + 1, tokens.end());
    } else {
        failRuntime("Number of tokens in header line of expression counts file " + expressionCountsFileName +
                    " is inconsistent with file contents.");
    }
    std::vector<std::pair<uint32_t, uint32_t>> cellsToBeKept;                 // (index in the meta data file, column - 1)
    std::vector<uint32_t> keptCellOfColumn(expectedTokenCount, kNone);
    for (size_t i = 0; i < cellNamesInExpressionCountsFile.size(); i++) {
        const auto it = metaDataInFileMap.find(cellNamesInExpressionCountsFile[i]);
        if (it == metaDataInFileMap.end()) continue;
        keptCellOfColumn[i + 1] = uint32_t(cellsToBeKept.size());
        cellsToBeKept.push_back(std::make_pair(it->second, uint32_t(i)));
    }
    const uint32_t keptCount = uint32_t(cellsToBeKept.size());
    if (uint64_t(cellCount()) + keptCount >= kNone - 1u) fail(EM2_ERROR_UNSUPPORTED, "addCells: the store is full (32-bit cell ids).");

    // The lines of the genes: where they are, and -- on the device path -- what the device says of them.
    const char* body = expressionReader.at;
    const uint64_t bodyBytes = uint64_t(expressionReader.end - body);
    std::vector<HostLine> lines;
    std::vector<CsvDeferred> deferred;                                        // .begin/.end unused here: see deferredRange
    std::vector<std::pair<uint64_t, uint64_t>> deferredRange;
    std::unique_ptr<CsvSession, void (*)(CsvSession*)> session(nullptr, csvSessionDestroy);
    if (chunkBytes == 0) chunkBytes = kDefaultCsvChunkBytes;
    if (chunkBytes > kMaxCsvChunkBytes) chunkBytes = kMaxCsvChunkBytes;
    std::vector<std::pair<uint64_t, uint64_t>> chunks;                        // whole lines, at most chunkBytes where a line allows
    if (useDevice && csvSeparatorsRunOnDevice(expressionCountsFileSeparators)) {
        for (uint64_t begin = 0; begin < bodyBytes;) {
            uint64_t end = bodyBytes;
            if (bodyBytes - begin > chunkBytes) {
                const void* last = ::memrchr(body + begin, '\n', size_t(chunkBytes));
                if (!last) last = std::memchr(body + begin + chunkBytes, '\n', size_t(bodyBytes - begin - chunkBytes));
                if (last) end = uint64_t(static_cast<const char*>(last) - body) + 1u;
            }
            if (end - begin > kMaxCsvChunkBytes) useDevice = false;           // a line the 32-bit offsets do not hold
            chunks.push_back(std::make_pair(begin, end));
            begin = end;
        }
    } else {
        useDevice = false;
    }
    if (useDevice) {
        session.reset(csvSessionCreate());
        std::vector<CsvLine> chunkLines;
        std::vector<CsvDeferred> chunkDeferred;
        for (const auto& chunk : chunks) {
            if (lines.size() >= kNone) fail(EM2_ERROR_UNSUPPORTED, "addCells: too many lines in " + expressionCountsFileName);
            const int rc = csvSessionChunk(session.get(), body + chunk.first, chunk.second - chunk.first, expressionCountsFileSeparators,
                                           uint32_t(expectedTokenCount), keptCellOfColumn, uint32_t(lines.size()), chunkLines,
                                           chunkDeferred);
            if (rc != EM2_OK) fail(rc, em2_last_error());
            for (const CsvLine& l : chunkLines) {
                lines.push_back(HostLine{chunk.first + l.begin, chunk.first + l.end, chunk.first + l.firstBegin, chunk.first + l.firstEnd,
                                         l.tokenCount, l.status});
            }
            for (const CsvDeferred& d : chunkDeferred) {
                deferred.push_back(d);
                deferredRange.push_back(std::make_pair(chunk.first + d.begin, chunk.first + d.end));
            }
        }
    } else {
        LineReader reader(body, size_t(bodyBytes));
        while (reader.next(line, length)) {
            const uint32_t status = length == 0 ? uint32_t(kCsvEmpty) : uint32_t(kCsvEscape);     // kCsvEscape: tokenized here, whole
            stripCr(line, length);
            const uint64_t begin = uint64_t(line - body);
            lines.push_back(HostLine{begin, begin + length, begin, begin, 0u, status});
        }
    }
    if (lines.size() >= kNone) fail(EM2_ERROR_UNSUPPORTED, "addCells: too many lines in " + expressionCountsFileName);
    if (deferredFieldCount) *deferredFieldCount = deferred.size();

    // The fields the device left open: their counts, or per line the first invalid one in the order of the kept cells.
    std::vector<CsvTriple> counts;
    std::map<uint32_t, std::pair<uint32_t, std::string>> invalidOfLine;
    for (size_t i = 0; i < deferred.size(); i++) {
        const CsvDeferred& d = deferred[i];
        tokenize(expressionCountsFileSeparators, body + deferredRange[i].first, size_t(deferredRange[i].second - deferredRange[i].first),
                 tokens, true);
        const std::string token = tokens.empty() ? std::string() : tokens[0];
        const uint32_t kept = keptCellOfColumn[d.column];
        float value = 0.f;
        const int kind = countOf(token, &value);
        if (kind == 1) {
            counts.push_back(CsvTriple{kept, d.line, value});
        } else if (kind == 2) {
            const auto it = invalidOfLine.find(d.line);
            if (it == invalidOfLine.end() || kept < it->second.first) invalidOfLine[d.line] = std::make_pair(kept, token);
        }
    }

    // The lines in file order (:559-626): the first error of the first failing line.
    std::set<std::string> geneNamesInFile;
    std::vector<std::string> newGenes;
    std::vector<uint32_t> geneIdOfLine(lines.size());
    const auto invalidCount = [&](const std::string& token, size_t lineIndex) {
        failRuntime("Invalid expression count " + (token.empty() ? std::string("(empty)") : token) + " encountered at line " +
                    std::to_string(lineIndex + 2u) + " of file " + expressionCountsFileName);
    };
    for (size_t i = 0; i < lines.size(); i++) {
        const HostLine& l = lines[i];
        if (l.status == kCsvEmpty) failRuntime("Empty line in expression counts file " + expressionCountsFileName);
        const bool onHost = l.status == kCsvEscape;
        std::string geneName;
        if (onHost) {
            tokenize(expressionCountsFileSeparators, body + l.begin, size_t(l.end - l.begin), tokens, true);
        } else {
            std::vector<std::string> first;
            tokenize(expressionCountsFileSeparators, body + l.firstBegin, size_t(l.firstEnd - l.firstBegin), first, true);
            if (!first.empty()) geneName = first[0];
        }
        if (onHost ? tokens.size() != expectedTokenCount : l.status == kCsvTokenCount) {
            failRuntime("Unexpected number of items in line of expression counts file " + expressionCountsFileName);
        }
        if (onHost) geneName = tokens[0];
        if (!geneNamesInFile.insert(geneName).second) {
            failRuntime("Duplicate entry for gene " + geneName + " in cell expression counts file " + expressionCountsFileName);
        }
        uint32_t geneId = s.geneNames.find(geneName);
        if (geneId == kInvalidStringId) {
            geneId = uint32_t(s.geneNames.size() + newGenes.size());
            newGenes.push_back(geneName);
        }
        geneIdOfLine[i] = geneId;
        if (onHost) {
            for (uint32_t k = 0; k < keptCount; k++) {
                const std::string& token = tokens[cellsToBeKept[k].second + 1u];
                float value = 0.f;
                const int kind = countOf(token, &value);
                if (kind == 2) invalidCount(token, i);
                if (kind == 1) counts.push_back(CsvTriple{k, uint32_t(i), value});
            }
        } else {
            const auto it = invalidOfLine.find(uint32_t(i));
            if (it != invalidOfLine.end()) invalidCount(it->second.second, i);
        }
    }
    if (s.geneNames.size() + newGenes.size() >= kNone) fail(EM2_ERROR_UNSUPPORTED, "addCells: the store is full (32-bit gene ids).");

    // addCell's storing part for every kept cell (:241-277).
    std::vector<uint32_t> status(keptCount, 0u);
    std::vector<uint64_t> toc(size_t(keptCount) + 1u, 0u);
    std::vector<em2_count> data;
    std::vector<CellRecord> cells(keptCount);
    if (useDevice) {
        bool failed = false;
        const int rc = csvSessionFinish(session.get(), counts, keptCount, uint32_t(lines.size()), geneIdOfLine, status, toc, data, cells,
                                        &failed);
        if (rc != EM2_OK) fail(rc, em2_last_error());
    } else {
        std::vector<std::vector<em2_count>> entriesOfCell(keptCount);
        for (const CsvTriple& t : counts) {                                   // appended in line order
            em2_count e;
            e.gene = geneIdOfLine[t.line];
            e.count = t.value;
            entriesOfCell[t.cell].push_back(e);
        }
        for (uint32_t k = 0; k < keptCount; k++) {
            uint32_t duplicateGene = kNone;
            status[k] = uint32_t(storeCell(entriesOfCell[k], cells[k], duplicateGene));
            data.insert(data.end(), entriesOfCell[k].begin(), entriesOfCell[k].end());
            toc[k + 1u] = data.size();
            std::vector<em2_count>().swap(entriesOfCell[k]);
        }
    }

    // addCell's checks, cell by cell (:181-215, :251-253), on the lists of :631-649.
    std::vector<MetaData> metaDataOfCell(keptCount);
    std::unordered_set<std::string> namesOfBatch;
    for (uint32_t k = 0; k < keptCount; k++) {
        MetaData& metaData = metaDataOfCell[k];
        metaData = additionalCellMetaData;
        const std::vector<std::string>& values = metaDataInFile[cellsToBeKept[k].first];
        for (size_t j = 0; j < metaDataNames.size(); j++) metaData.push_back(std::make_pair(metaDataNames[j], values[j]));
        for (auto& p : metaData) {                                            // :190-197
            if (p.first == "CellName") {
                std::swap(p, metaData.front());
                break;
            }
        }
        const std::string& cellName = metaData.front().second;
        if (s.cellNames.find(cellName) != kInvalidStringId || !namesOfBatch.insert(cellName).second) {
            failRuntime("Cell name " + cellName + " already exists.");
        }
        if (status[k] == kIngestNegative) failRuntime("Negative expression count encountered.");
        if (status[k] != kIngestOk) failRuntime("addCells: the storing pass reports status " + std::to_string(status[k]));
    }

    firstCellId = cellCount();
    addedCellCount = writeCells(newGenes, keptCount, [&](size_t k) { return &metaDataOfCell[k]; }, toc.data(), data.data(), cells.data());
}

void Matrix::addCellMetaDataFromFile(const std::string& cellMetaDataFileName)
{
    const IngestState& s = ingest("addCellMetaData");
    const MappedText file(cellMetaDataFileName);
    if (!file.ok) failRuntime("Error opening " + cellMetaDataFileName);
    LineReader reader(file.p, file.bytes);
    const char* line;
    size_t length;
    if (!reader.next(line, length)) failRuntime("Error reading the header line from file " + cellMetaDataFileName);
    std::vector<std::string> metaDataNames, metaDataValues;
    tokenize(",", line, length, metaDataNames, true);
    if (metaDataNames.empty()) failRuntime("Invalid format of cell meta data file " + cellMetaDataFileName);
    struct Item {
        uint32_t cellId;
        size_t field;
        std::string value;
    };
    std::vector<Item> items;                                                  // checked first, written after: all or nothing
    while (reader.next(line, length)) {
        tokenize(",", line, length, metaDataValues, true);
        if (metaDataValues.size() != metaDataNames.size()) failRuntime("Unexpected number of meta data values in " + cellMetaDataFileName);
        const std::string& cellName = metaDataValues.front();
        const uint32_t cellId = s.cellNames.find(cellName);
        if (cellId == kInvalidStringId) failRuntime("Attempt to add meta data for undefined cell " + cellName);
        for (size_t i = 1; i < metaDataNames.size(); i++) {
            if (!metaDataNames[i].empty()) items.push_back(Item{cellId, i, metaDataValues[i]});
        }
    }
    for (const Item& item : items) setCellMetaData(item.cellId, metaDataNames[item.field], item.value);
}

}  // namespace host
}  // namespace em2
