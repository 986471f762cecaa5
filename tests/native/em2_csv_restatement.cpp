// em2_csv_restatement.cpp -- what the reference does with the two files of addCells and the one of addCellMetaData, restated
// for the tests with the reference's containers (std::map, std::set, vector<vector<string>>), its getline loops and a strtof
// per field, and without a store: the output is the sequence of addGene / addCell / setCellMetaData calls the reference
// would make, or the text of the error it would throw.  Test infrastructure only; nothing of the product is linked.
//
// Output: fields that end in NUL.
//   "G" name                                          addGene(name)
//   "C" pairCount (name value)* countCount (gene bits)*    addCell(metaData, counts); bits = the float's 8 hex digits
//   "M" cellName name value                           setCellMetaData(cell of that name, name, value)
//   "T" token                                         a token (em2r_csv_tokenize)
//   "E" text                                          the error; nothing follows
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

using std::map;
using std::pair;
using std::runtime_error;
using std::set;
using std::string;
using std::vector;

namespace {

string output;

void put(const string& field)
{
    output += field;
    output += '\0';
}

// boost::escaped_list_separator<char>("\\", separators, "\"") as boost::tokenizer drives it, then boost::algorithm::trim.
void tokenize(const string& separators, const string& inputString, vector<string>& tokens, bool removeLeadingAndTrailingBlanks)
{
    tokens.clear();
    string::const_iterator next = inputString.begin();
    const string::const_iterator end = inputString.end();
    bool lastWasSeparator = false;
    while (true) {                                         // one token per round
        string token;
        bool inQuote = false;
        if (next == end) {
            if (!lastWasSeparator) break;
            lastWasSeparator = false;
            tokens.push_back(token);
            break;
        }
        lastWasSeparator = false;
        bool tokenEnded = false;
        for (; next != end; ++next) {
            if (*next == '\\') {
                if (++next == end) throw runtime_error("cannot end with escape");
                if (*next == 'n') token += '\n';
                else if (*next == '"' || separators.find(*next) != string::npos || *next == '\\') token += *next;
                else throw runtime_error("unknown escape sequence");
            } else if (separators.find(*next) != string::npos) {
                if (!inQuote) {
                    ++next;
                    lastWasSeparator = true;
                    tokenEnded = true;
                    break;
                }
                token += *next;
            } else if (*next == '"') {
                inQuote = !inQuote;
            } else {
                token += *next;
            }
        }
        tokens.push_back(token);
        if (!tokenEnded) break;
    }
    if (removeLeadingAndTrailingBlanks) {
        for (string& token : tokens) {
            const char* blanks = " \t\n\v\f\r";
            const size_t first = token.find_first_not_of(blanks);
            if (first == string::npos) {
                token.clear();
            } else {
                token = token.substr(first, token.find_last_not_of(blanks) - first + 1);
            }
        }
    }
}

size_t countTokensInSecondLine(const string& fileName, const string& separators, const char* what)
{
    std::ifstream file(fileName);
    if (!file) throw runtime_error("Could not open file " + fileName);
    string line;
    std::getline(file, line);
    if (!file) throw runtime_error("Error reading header line of file " + fileName);
    std::getline(file, line);
    if (!file) throw runtime_error("Error reading the second line of file " + fileName);
    if (line.empty()) throw runtime_error(string("Empty line in ") + what + " file " + fileName);    // the stated departure
    if (line[line.size() - 1] == 13) line.resize(line.size() - 1);
    vector<string> tokens;
    tokenize(separators, line, tokens, false);
    return tokens.size();
}

void addCells(const string& expressionCountsFileName, const string& expressionCountsFileSeparators, const string& cellMetaDataFileName,
              const string& cellMetaDataFileSeparators, const vector<pair<string, string>>& additionalCellMetaData)
{
    const size_t metaDataCount = countTokensInSecondLine(cellMetaDataFileName, cellMetaDataFileSeparators, "cell meta data");
    std::ifstream metaDataFile(cellMetaDataFileName);
    if (!metaDataFile) throw runtime_error("Error opening cell meta data file " + cellMetaDataFileName);
    string line;
    std::getline(metaDataFile, line);
    if (line.empty()) throw runtime_error("Error reading header line from cell meta data file " + cellMetaDataFileName);
    if (line[line.size() - 1] == 13) line.resize(line.size() - 1);
    vector<string> tokens;
    tokenize(cellMetaDataFileSeparators, line, tokens, false);
    vector<string> metaDataNames;
    metaDataNames.push_back("CellName");
    if (tokens.size() == metaDataCount) {
        for (size_t i = 1; i < tokens.size(); i++) metaDataNames.push_back(tokens[i]);
    } else if (tokens.size() == metaDataCount - 1) {
        for (size_t i = 0; i < tokens.size(); i++) metaDataNames.push_back(tokens[i]);
    } else {
        throw runtime_error("Number of tokens in header line of cell meta data file " + cellMetaDataFileName +
                            " is inconsistent with file contents.");
    }

    vector<vector<string>> metaDataInFile;
    map<string, uint32_t> metaDataInFileMap;
    while (true) {
        std::getline(metaDataFile, line);
        if (!metaDataFile) break;
        if (line.empty()) throw runtime_error("Empty line in cell meta data file " + cellMetaDataFileName);
        if (line[line.size() - 1] == 13) line.resize(line.size() - 1);
        tokens.clear();
        tokenize(cellMetaDataFileSeparators, line, tokens, false);
        if (tokens.size() != metaDataNames.size()) {
            throw runtime_error("Unexpected number of items in line of cell meta data file " + cellMetaDataFileName);
        }
        const string& cellName = tokens[0];
        if (metaDataInFileMap.find(cellName) != metaDataInFileMap.end()) {
            throw runtime_error("Duplicate cell name " + cellName + " in cell meta data file " + cellMetaDataFileName);
        }
        metaDataInFileMap.insert(std::make_pair(cellName, uint32_t(metaDataInFile.size())));
        metaDataInFile.push_back(tokens);
    }

    const size_t cellCountInExpressionFile =
        countTokensInSecondLine(expressionCountsFileName, expressionCountsFileSeparators, "expression counts") - 1;
    std::ifstream expressionCountsFile(expressionCountsFileName);
    if (!expressionCountsFile) throw runtime_error("Error opening expression counts file " + expressionCountsFileName);
    std::getline(expressionCountsFile, line);
    if (line.empty()) throw runtime_error("Error reading header line from expression counts file " + expressionCountsFileName);
    if (line[line.size() - 1] == 13) line.resize(line.size() - 1);
    tokenize(expressionCountsFileSeparators, line, tokens, true);
    vector<string> cellNamesInExpressionCountsFile;
    if (tokens.size() == cellCountInExpressionFile) {
        cellNamesInExpressionCountsFile = tokens;
    } else if (tokens.size() == cellCountInExpressionFile + 1) {
        for (size_t i = 1; i < tokens.size(); i++) cellNamesInExpressionCountsFile.push_back(tokens[i]);
    } else {
        throw runtime_error("Number of tokens in header line of expression counts file " + expressionCountsFileName +
                            " is inconsistent with file contents.");
    }

    vector<pair<uint32_t, uint32_t>> cellsToBeKept;        // (index in the meta data file, index in the expression counts file)
    for (size_t i = 0; i < cellNamesInExpressionCountsFile.size(); i++) {
        const auto it = metaDataInFileMap.find(cellNamesInExpressionCountsFile[i]);
        if (it == metaDataInFileMap.end()) continue;
        cellsToBeKept.push_back(std::make_pair(it->second, uint32_t(i)));
    }

    set<string> geneNamesInFile;
    vector<string> geneNameOfLine;
    vector<vector<pair<uint32_t, float>>> counts(cellsToBeKept.size());       // (gene line, count)
    while (true) {
        std::getline(expressionCountsFile, line);
        if (!expressionCountsFile) break;
        if (line.empty()) throw runtime_error("Empty line in expression counts file " + expressionCountsFileName);
        if (line[line.size() - 1] == 13) line.resize(line.size() - 1);
        tokens.clear();
        tokenize(expressionCountsFileSeparators, line, tokens, true);
        if (tokens.size() != cellCountInExpressionFile + 1) {
            throw runtime_error("Unexpected number of items in line of expression counts file " + expressionCountsFileName);
        }
        const string& geneName = tokens[0];
        if (geneNamesInFile.find(geneName) != geneNamesInFile.end()) {
            throw runtime_error("Duplicate entry for gene " + geneName + " in cell expression counts file " + expressionCountsFileName);
        }
        geneNamesInFile.insert(geneName);
        put("G");
        put(geneName);
        geneNameOfLine.push_back(geneName);
        for (size_t i = 0; i < cellsToBeKept.size(); i++) {
            const string& countString = tokens[cellsToBeKept[i].second + 1];
            if (countString == "0" || countString == "0.") continue;
            const char* countStringBegin = countString.c_str();
            char* check = const_cast<char*>(countStringBegin + countString.size());
            const float count = strtof(countStringBegin, &check);
            if (check == countStringBegin) {
                throw runtime_error("Invalid expression count " + (countString.empty() ? "(empty)" : countString) +
                                    " encountered at line " + std::to_string(geneNamesInFile.size() + 1) + " of file " +
                                    expressionCountsFileName);
            }
            counts[i].push_back(std::make_pair(uint32_t(geneNameOfLine.size() - 1), count));
        }
    }

    vector<pair<string, string>> metaDataForOneCell = additionalCellMetaData;
    for (const string& metaDataName : metaDataNames) metaDataForOneCell.push_back(std::make_pair(metaDataName, ""));
    for (size_t i = 0; i < cellsToBeKept.size(); i++) {
        for (size_t j = 0; j < metaDataNames.size(); j++) {
            metaDataForOneCell[j + additionalCellMetaData.size()].second = metaDataInFile[cellsToBeKept[i].first][j];
        }
        put("C");
        put(std::to_string(metaDataForOneCell.size()));
        for (const auto& p : metaDataForOneCell) {
            put(p.first);
            put(p.second);
        }
        put(std::to_string(counts[i].size()));
        for (const auto& p : counts[i]) {
            put(geneNameOfLine[p.first]);
            uint32_t bits;
            std::memcpy(&bits, &p.second, 4);
            char hex[16];
            std::snprintf(hex, sizeof(hex), "%08x", bits);
            put(hex);
        }
    }
}

void addCellMetaData(const string& cellMetaDataFileName, const set<string>& cellNames)
{
    std::ifstream cellMetaDataFile(cellMetaDataFileName);
    if (!cellMetaDataFile) throw runtime_error("Error opening " + cellMetaDataFileName);
    string line;
    std::getline(cellMetaDataFile, line);
    if (!cellMetaDataFile) throw runtime_error("Error reading the header line from file " + cellMetaDataFileName);
    vector<string> metaDataNames;
    tokenize(",", line, metaDataNames, true);
    if (metaDataNames.size() == 0) throw runtime_error("Invalid format of cell meta data file " + cellMetaDataFileName);
    vector<string> metaDataValues;
    while (true) {
        std::getline(cellMetaDataFile, line);
        if (!cellMetaDataFile) break;
        tokenize(",", line, metaDataValues, true);
        if (metaDataValues.size() != metaDataNames.size()) {
            throw runtime_error("Unexpected number of meta data values in " + cellMetaDataFileName);
        }
        const string& cellName = metaDataValues.front();
        if (cellNames.find(cellName) == cellNames.end()) throw runtime_error("Attempt to add meta data for undefined cell " + cellName);
        for (size_t i = 1; i < metaDataNames.size(); i++) {
            if (metaDataNames[i].size() > 0) {
                put("M");
                put(cellName);
                put(metaDataNames[i]);
                put(metaDataValues[i]);
            }
        }
    }
}

vector<string> unpack(const char* packed, uint64_t bytes)
{
    vector<string> strings;
    for (uint64_t at = 0; at < bytes;) {
        const size_t length = std::strlen(packed + at);
        strings.push_back(string(packed + at, length));
        at += length + 1;
    }
    return strings;
}

template <class F> const char* run(F f, uint64_t* bytes)
{
    output.clear();
    try {
        f();
    } catch (const std::exception& e) {
        output.clear();
        put("E");
        put(e.what());
    }
    *bytes = output.size();
    return output.data();
}

}  // namespace

extern "C" {

const char* em2r_csv_tokenize(const char* separators, const char* line, uint64_t lineBytes, int trim, uint64_t* bytes)
{
    return run(
        [&] {
            vector<string> tokens;
            tokenize(separators, string(line, size_t(lineBytes)), tokens, trim != 0);
            for (const string& token : tokens) {
                put("T");
                put(token);
            }
        },
        bytes);
}

const char* em2r_csv_add_cells(const char* expressionCountsFileName, const char* expressionCountsFileSeparators,
                               const char* cellMetaDataFileName, const char* cellMetaDataFileSeparators, const char* additional,
                               uint64_t additionalBytes, uint64_t* bytes)
{
    return run(
        [&] {
            const vector<string> flat = unpack(additional, additionalBytes);
            vector<pair<string, string>> pairs;
            for (size_t i = 0; i + 1 < flat.size(); i += 2) pairs.push_back(std::make_pair(flat[i], flat[i + 1]));
            addCells(expressionCountsFileName, expressionCountsFileSeparators, cellMetaDataFileName, cellMetaDataFileSeparators, pairs);
        },
        bytes);
}

const char* em2r_csv_add_cell_meta_data(const char* cellMetaDataFileName, const char* cellNames, uint64_t cellNamesBytes, uint64_t* bytes)
{
    return run(
        [&] {
            const vector<string> names = unpack(cellNames, cellNamesBytes);
            addCellMetaData(cellMetaDataFileName, set<string>(names.begin(), names.end()));
        },
        bytes);
}

}  // extern "C"
