// em2_csv.h -- addCells from an expression counts file and a cell meta data file (src/ExpressionMatrix.cpp:380-654), and
// addCellMetaData (src/ExpressionMatrixBioHub.cpp:337-392): the tokenizer and the line reader restated on the host
// (em2_csv_host.cpp) and the device pass over the text of the expression counts file (em2_csv.hip).
#ifndef EM2_CSV_H
#define EM2_CSV_H

#include "em2_ingest.h"

#include <string>
#include <vector>

namespace em2 {
namespace host {

// tokenize (src/tokenize.cpp:16-35): boost::escaped_list_separator<char>("\\", separators, "\"") over [line, line + length),
// then boost::algorithm::trim of every token where `trim` is set.  Throws Error(EM2_ERROR_RUNTIME) "cannot end with escape"
// and "unknown escape sequence".
void tokenize(const std::string& separators, const char* line, size_t length, std::vector<std::string>& tokens, bool trim);

// std::getline over a text in memory: lines end at '\n' whatever the quotes say, a last line without '\n' counts, a text
// that ends in '\n' has no extra empty line.
struct LineReader {
    const char* at;
    const char* end;
    LineReader(const char* text, size_t bytes) : at(text), end(text + bytes) {}
    bool next(const char*& line, size_t& length);
};

// What the device says of a line.  Offsets are bytes from the start of the text it was given; [begin, end) excludes the
// '\n' and one '\r' before it.  kCsvEscape: the line holds a '\\' and the device has emitted nothing else for it.
enum { kCsvOk = 0, kCsvEmpty = 1, kCsvTokenCount = 2, kCsvEscape = 3 };
struct CsvLine {
    uint32_t begin, end, tokenCount, status, firstBegin, firstEnd;
};
struct CsvDeferred {                                       // a field of a kept column the device does not decide
    uint32_t line, column, begin, end;
};
struct CsvTriple {                                         // a count the host has decided (kept cell, line, value)
    uint32_t cell, line;
    float value;
};

// The device side of one addCells call: the decided counts of all chunks stay on the device until finish().
struct CsvSession;
CsvSession* csvSessionCreate();
void csvSessionDestroy(CsvSession* session);
// One chunk of whole lines.  lines: offsets relative to `text`; deferred: line numbers include lineBase.  Returns an EM2
// status with the last error set.
int csvSessionChunk(CsvSession* session, const char* text, uint64_t bytes, const std::string& separators, uint32_t expectedTokens,
                    const std::vector<uint32_t>& keptCellOfColumn, uint32_t lineBase, std::vector<CsvLine>& lines,
                    std::vector<CsvDeferred>& deferred);
// Adds the host's counts, sorts by (cell, line), and runs em2_dev_ingest_count / _fill on the result.  Outputs as
// ingestChunkOnDevice's.
int csvSessionFinish(CsvSession* session, const std::vector<CsvTriple>& extra, uint32_t keptCellCount, uint32_t lineCount,
                     const std::vector<uint32_t>& geneIdOfLine, std::vector<uint32_t>& status, std::vector<uint64_t>& toc,
                     std::vector<em2_count>& data, std::vector<CellRecord>& cells, bool* failed);

// A separator string the device pass takes: 1 to 8 bytes, none of them '"', '\\', '\n' or '\r'.
bool csvSeparatorsRunOnDevice(const std::string& separators);

}  // namespace host
}  // namespace em2

#endif
