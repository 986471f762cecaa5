// em2_meta_data_restatement.cpp -- the reference's cell meta data semantics restated with standard containers, for the tests:
//   * the store as a std::list of (name id, value id) per cell, string tables as std::vector<std::string> + std::map (ids in
//     order of first insertion), usage counts (src/ExpressionMatrix.cpp:880-1029);
//   * createCellSetUsingMetaData (:1560-1622), one std::regex_match or string comparison per cell;
//   * histogramMetaData (:1301-1323) with a std::map<string, size_t> and the reference's comparator, the dense
//     vector<vector<size_t>> contingency table filled through two std::map<string, size_t> (:1358-1381), and computeRandIndex
//     (src/randIndex.hpp:24-98) with its loops in their own order and types;
//   * the contingency table of two integer labelings with a std::map, for the device entry.
// Test infrastructure only: nothing here is shared with the library.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <numeric>
#include <regex>
#include <string>
#include <utility>
#include <vector>

namespace {

using std::map;
using std::pair;
using std::string;
using std::vector;

const uint32_t kInvalid = 0xffffffffu;

struct Table {
    vector<string> strings;
    map<string, uint32_t> ids;
    uint32_t find(const string& s) const
    {
        const auto it = ids.find(s);
        return it == ids.end() ? kInvalid : it->second;
    }
    uint32_t insert(const string& s)
    {
        const auto it = ids.find(s);
        if (it != ids.end()) return it->second;
        const uint32_t id = uint32_t(strings.size());
        strings.push_back(s);
        ids[s] = id;
        return id;
    }
};

struct Store {
    vector<std::list<pair<uint32_t, uint32_t>>> cells;
    Table names, values;
    vector<uint32_t> usage;

    string value(uint32_t cell, uint32_t nameId) const       // getCellMetaData(CellId, StringId), :890-907
    {
        for (const auto& p : cells[cell]) {
            if (p.first == nameId) return p.second == kInvalid ? "" : values.strings[p.second];
        }
        return "";
    }
};

// src/randIndex.hpp:24-98, T = size_t.
void computeRandIndex(const vector<vector<size_t>>& contingencyTable, double& randIndex, double& adjustedRandIndex)
{
    const size_t columnCount = contingencyTable.front().size();
    vector<size_t> rowTotals;
    for (const auto& row : contingencyTable) rowTotals.push_back(std::accumulate(row.begin(), row.end(), 0ULL));
    vector<size_t> columnTotals(columnCount, 0.);
    for (const auto& row : contingencyTable) {
        for (size_t column = 0; column < columnCount; column++) columnTotals[column] += row[column];
    }
    const size_t n = std::accumulate(rowTotals.begin(), rowTotals.end(), 0ULL);
    const double nDouble = double(n);
    const double nBinomial2 = 0.5 * nDouble * (nDouble - 1.);
    double a = 0.;
    for (const auto& row : contingencyTable) {
        for (const size_t& value : row) {
            const double v = double(value);
            a += v * (v - 1.);
        }
    }
    a /= 2.;
    double b = -a;
    for (const auto rowTotal : rowTotals) {
        const double t = double(rowTotal);
        b += 0.5 * t * (t - 1.);
    }
    double c = -a;
    for (const auto columnTotal : columnTotals) {
        const double t = double(columnTotal);
        c += 0.5 * t * (t - 1.);
    }
    const double d = nBinomial2 - a - b - c;
    randIndex = (a + d) / (a + b + c + d);
    const double commonTerm = (a + b) * (a + c) + (c + d) * (b + d);
    const double adjustedRandIndexNumerator = nBinomial2 * (a + d) - commonTerm;
    const double adjustedRandIndexDenominator = nBinomial2 * nBinomial2 - commonTerm;
    adjustedRandIndex = adjustedRandIndexNumerator / adjustedRandIndexDenominator;
}

// OrderPairsBySecondGreaterThenByFirstLess (src/orderPairs.hpp).
bool histogramOrder(const pair<string, size_t>& x, const pair<string, size_t>& y)
{
    if (x.second > y.second) return true;
    if (y.second > x.second) return false;
    return x.first < y.first;
}

void histogramMetaData(const Store& store, const uint32_t* cellSet, uint64_t n, uint32_t nameId, vector<pair<string, size_t>>& sorted)
{
    map<string, size_t> histogram;
    for (uint64_t i = 0; i < n; i++) {
        const string metaDataValue = store.value(cellSet[i], nameId);
        const auto it = histogram.find(metaDataValue);
        if (it == histogram.end()) histogram.insert(std::make_pair(metaDataValue, 1));
        else ++(it->second);
    }
    sorted.clear();
    std::copy(histogram.begin(), histogram.end(), std::back_inserter(sorted));
    std::sort(sorted.begin(), sorted.end(), histogramOrder);
}

struct MetaDataTable {
    vector<pair<string, size_t>> histogram[2];
    vector<vector<size_t>> matrix;
    double randIndex = 0., adjustedRandIndex = 0.;
};

struct Contingency {
    vector<uint64_t> rowTotals, columnTotals, count;
    vector<uint32_t> i0, i1;
    uint64_t sums[3] = {0, 0, 0};
};

size_t packStrings(const vector<pair<string, size_t>>& histogram, char* out)
{
    size_t bytes = 0;
    for (const auto& p : histogram) {
        if (out) std::memcpy(out + bytes, p.first.c_str(), p.first.size() + 1);
        bytes += p.first.size() + 1;
    }
    return bytes;
}

}  // namespace

extern "C" {

void* em2r_md_create(uint32_t cellCount)
{
    Store* s = new Store;
    s->cells.resize(cellCount);
    return s;
}

void em2r_md_free(void* store) { delete static_cast<Store*>(store); }

// setCellMetaData, :942-967.
void em2r_md_set(void* store, uint32_t cell, const char* name, const char* value)
{
    Store& s = *static_cast<Store*>(store);
    const uint32_t nameId = s.names.insert(name);
    const uint32_t valueId = s.values.insert(value);
    for (auto& p : s.cells[cell]) {
        if (p.first == nameId) {
            p.second = valueId;
            return;
        }
    }
    s.cells[cell].push_back(std::make_pair(nameId, valueId));
    if (s.usage.size() <= nameId) s.usage.push_back(1);
    else ++s.usage[nameId];
}

// removeCellMetaData, :998-1029, for the cells of a set.
void em2r_md_remove(void* store, const uint32_t* cellSet, uint64_t n, const char* name)
{
    Store& s = *static_cast<Store*>(store);
    const uint32_t nameId = s.names.find(name);
    if (nameId == kInvalid) return;
    for (uint64_t i = 0; i < n; i++) {
        auto& l = s.cells[cellSet[i]];
        for (auto it = l.begin(); it != l.end(); ++it) {
            if (it->first == nameId) {
                --s.usage[nameId];
                l.erase(it);
                break;
            }
        }
    }
}

// The usage count of a name, -1 for a name the table does not hold.
int64_t em2r_md_usage(void* store, const char* name)
{
    const Store& s = *static_cast<Store*>(store);
    const uint32_t nameId = s.names.find(name);
    return nameId == kInvalid ? -1 : int64_t(s.usage[nameId]);
}

// getCellMetaData(cellId, name), :880-889: the bytes of the value; copied when out is given.
uint64_t em2r_md_value(void* store, uint32_t cell, const char* name, char* out)
{
    const Store& s = *static_cast<Store*>(store);
    const uint32_t nameId = s.names.find(name);
    const string v = nameId == kInvalid ? string() : s.value(cell, nameId);
    if (out) std::memcpy(out, v.data(), v.size());
    return v.size();
}

// getCellMetaData(cellId), :913-922: name, 0, value, 0, ...
uint64_t em2r_md_pairs(void* store, uint32_t cell, char* out)
{
    const Store& s = *static_cast<Store*>(store);
    string all;
    for (const auto& p : s.cells[cell]) {
        all.append(s.names.strings[p.first]).push_back('\0');
        all.append(s.values.strings[p.second]).push_back('\0');
    }
    if (out) std::memcpy(out, all.data(), all.size());
    return all.size();
}

// createCellSetUsingMetaData, :1572-1616, over all cells: the ids into out[cellCount]; -1 where std::regex throws.
int64_t em2r_md_select(void* store, const char* metaDataFieldName, const char* matchStringC, int useRegex, uint32_t* out)
{
    const Store& s = *static_cast<Store*>(store);
    const string matchString = matchStringC;
    std::regex regex;
    try {
        if (useRegex) regex = matchString;
    } catch (const std::regex_error&) {
        return -1;
    }
    int64_t count = 0;
    for (uint32_t cellId = 0; cellId < s.cells.size(); cellId++) {
        for (const pair<uint32_t, uint32_t>& p : s.cells[cellId]) {
            if (s.names.strings[p.first] != metaDataFieldName) continue;
            const string& metaDataValue = s.values.strings[p.second];
            bool includeThisCell;
            if (useRegex) {
                includeThisCell = std::regex_match(metaDataValue.begin(), metaDataValue.end(), regex);
            } else {
                includeThisCell = (metaDataValue.size() == matchString.size()) &&
                                  std::equal(matchString.begin(), matchString.end(), metaDataValue.begin());
            }
            if (includeThisCell) out[count++] = cellId;
            break;
        }
    }
    return count;
}

// histogramMetaData of one field (name1 == NULL) or computeMetaDataRandIndex's histograms, table and indices of two (:1350-1387).
void* em2r_md_table(void* store, const uint32_t* cellSet, uint64_t n, const char* name0, const char* name1)
{
    const Store& s = *static_cast<Store*>(store);
    MetaDataTable* t = new MetaDataTable;
    const uint32_t nameId0 = s.names.find(name0);
    histogramMetaData(s, cellSet, n, nameId0, t->histogram[0]);
    if (!name1) return t;
    const uint32_t nameId1 = s.names.find(name1);
    histogramMetaData(s, cellSet, n, nameId1, t->histogram[1]);
    const size_t n0 = t->histogram[0].size(), n1 = t->histogram[1].size();
    map<string, size_t> map0, map1;
    for (size_t i = 0; i < n0; i++) map0.insert(std::make_pair(t->histogram[0][i].first, i));
    for (size_t i = 0; i < n1; i++) map1.insert(std::make_pair(t->histogram[1][i].first, i));
    t->matrix.assign(n0, vector<size_t>(n1, 0));
    for (uint64_t i = 0; i < n; i++) {
        const string metaDataValue0 = s.value(cellSet[i], nameId0);
        const string metaDataValue1 = s.value(cellSet[i], nameId1);
        ++(t->matrix[map0[metaDataValue0]][map1[metaDataValue1]]);
    }
    computeRandIndex(t->matrix, t->randIndex, t->adjustedRandIndex);
    return t;
}

void em2r_md_table_sizes(void* table, uint64_t* n0, uint64_t* n1, uint64_t* bytes0, uint64_t* bytes1)
{
    const MetaDataTable& t = *static_cast<MetaDataTable*>(table);
    *n0 = t.histogram[0].size();
    *n1 = t.histogram[1].size();
    *bytes0 = packStrings(t.histogram[0], nullptr);
    *bytes1 = packStrings(t.histogram[1], nullptr);
}

// dense: n0 * n1 counts, row by row (NULL where only the histograms are wanted); indices: randIndex, adjustedRandIndex.
void em2r_md_table_get(void* table, char* values0, uint64_t* counts0, char* values1, uint64_t* counts1, uint64_t* dense, double* indices)
{
    const MetaDataTable& t = *static_cast<MetaDataTable*>(table);
    packStrings(t.histogram[0], values0);
    packStrings(t.histogram[1], values1);
    for (size_t i = 0; i < t.histogram[0].size(); i++) counts0[i] = t.histogram[0][i].second;
    for (size_t i = 0; i < t.histogram[1].size(); i++) counts1[i] = t.histogram[1][i].second;
    if (dense) {
        size_t at = 0;
        for (const auto& row : t.matrix) {
            for (const size_t v : row) dense[at++] = v;
        }
    }
    indices[0] = t.randIndex;
    indices[1] = t.adjustedRandIndex;
}

void em2r_md_table_free(void* table) { delete static_cast<MetaDataTable*>(table); }

// computeRandIndex on a dense table[rows][columns].
void em2r_rand_index(const uint64_t* table, uint64_t rows, uint64_t columns, double* indices)
{
    vector<vector<size_t>> matrix(rows, vector<size_t>(columns, 0));
    for (uint64_t r = 0; r < rows; r++) {
        for (uint64_t c = 0; c < columns; c++) matrix[r][c] = table[r * columns + c];
    }
    computeRandIndex(matrix, indices[0], indices[1]);
}

// The contingency table of two integer labelings, kept in a std::map; the three sums in 64-bit integers.
void* em2r_contingency(const uint32_t* id0, const uint32_t* id1, uint64_t n, uint32_t n0, uint32_t n1)
{
    Contingency* c = new Contingency;
    c->rowTotals.assign(n0, 0);
    c->columnTotals.assign(n1, 0);
    map<pair<uint32_t, uint32_t>, uint64_t> cells;
    for (uint64_t i = 0; i < n; i++) {
        ++cells[std::make_pair(id0[i], id1[i])];
        ++c->rowTotals[id0[i]];
        ++c->columnTotals[id1[i]];
    }
    for (const auto& cell : cells) {
        c->i0.push_back(cell.first.first);
        c->i1.push_back(cell.first.second);
        c->count.push_back(cell.second);
        c->sums[0] += cell.second * (cell.second - 1);
    }
    for (const uint64_t t : c->rowTotals) c->sums[1] += t * (t - 1);
    for (const uint64_t t : c->columnTotals) c->sums[2] += t * (t - 1);
    return c;
}

uint64_t em2r_contingency_size(void* contingency) { return static_cast<Contingency*>(contingency)->count.size(); }

void em2r_contingency_get(void* contingency, uint64_t* rowTotals, uint64_t* columnTotals, uint32_t* i0, uint32_t* i1, uint64_t* count,
                          uint64_t* sums)
{
    const Contingency& c = *static_cast<Contingency*>(contingency);
    std::copy(c.rowTotals.begin(), c.rowTotals.end(), rowTotals);
    std::copy(c.columnTotals.begin(), c.columnTotals.end(), columnTotals);
    std::copy(c.i0.begin(), c.i0.end(), i0);
    std::copy(c.i1.begin(), c.i1.end(), i1);
    std::copy(c.count.begin(), c.count.end(), count);
    std::copy(c.sums, c.sums + 3, sums);
}

void em2r_contingency_free(void* contingency) { delete static_cast<Contingency*>(contingency); }

}  // extern "C"
