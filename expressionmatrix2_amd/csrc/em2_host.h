// em2_host.h -- host side of the boundary: the reference's memory-mapped file formats and the
// ExpressionMatrix-level drivers of the LSH path (name lookup, subset construction, result files).
//
// File formats (all little-endian, written by mmap in the reference):
//   MemoryMapped::Vector<T>   src/MemoryMappedVector.hpp:141-197   256-byte header {headerSize, objectSize,
//                             objectCount, pageCount, fileSize, capacity, magic 0xa3756fd4b5d8bcc1, 25 zero words}
//                             + objectCount objects; file size rounded up to 4096.
//   MemoryMapped::Object<T>   src/MemoryMappedObject.hpp:88-140    same header with magic 0xb7756f4515d8bc94,
//                             objectCount = capacity = 1.
//   VectorOfVectors<T,Int>    src/MemoryMappedVectorOfVectors.hpp:29-34  <name>.toc (Vector<Int>, n+1 offsets)
//                             + <name>.data (Vector<T>).
#ifndef EM2_HOST_H
#define EM2_HOST_H

#include <stdint.h>
#include <map>
#include <functional>
#include <string>
#include <vector>

#include "../../include/em2_lsh.h"

namespace em2 {
namespace host {

// Thrown for every condition the reference reports with std::runtime_error; .what() is the reference's text
// where the reference has one.
struct Error {
    int code;
    std::string message;
};

class MetaDataStore;       // em2_meta_data.h
struct MetaDataTable;
struct IngestState;        // em2_ingest.h

// A read-only or writable mapping of one MemoryMapped file.
class MappedFile {
public:
    MappedFile() : base_(nullptr), size_(0), writable_(false) {}
    ~MappedFile() { close(); }
    MappedFile(const MappedFile&) = delete;
    MappedFile& operator=(const MappedFile&) = delete;

    void openExisting(const std::string& path, bool isObject, size_t objectSize, bool writable = false);
    void createNew(const std::string& path, bool isObject, size_t objectSize, size_t objectCount);
    void close();
    // MemoryMapped::Vector::push_back / resize (src/MemoryMappedVector.hpp:575-640) for a vector that was created here or
    // opened writable: the file grows to at least twice its capacity when it is full (the reference: 1.5 times), new objects
    // of resize are zero.  data() may move.
    void append(const void* objects, size_t count);
    void resize(size_t objectCount);
    bool isWritable() const { return writable_; }

    bool isOpen() const { return base_ != nullptr; }
    size_t objectCount() const;
    const void* data() const { return static_cast<const char*>(base_) + 256; }
    void* data() { return static_cast<char*>(base_) + 256; }

private:
    void reserve(size_t capacity);
    void* base_;
    size_t size_;
    bool writable_;
    std::string path_;
};

void removeFile(const std::string& path);
bool fileExists(const std::string& path);

// GeneSet (src/GeneSet.hpp:62-77): sorted global ids + table global id -> local id (0xffffffff = absent).
struct GeneSet {
    MappedFile globalIds;
    MappedFile localIds;
    uint32_t size() const { return uint32_t(globalIds.objectCount()); }
    const uint32_t* genes() const { return static_cast<const uint32_t*>(globalIds.data()); }
    uint32_t localId(uint32_t globalId) const
    {
        return globalId < localIds.objectCount() ? static_cast<const uint32_t*>(localIds.data())[globalId] : 0xffffffffu;
    }
};

// The part of ExpressionMatrix (src/ExpressionMatrix.hpp:80-1247) the LSH path touches.
class Matrix {
public:
    explicit Matrix(const std::string& directoryName);       // accessExisting, ExpressionMatrix.cpp:109-160
    ~Matrix();

    const std::string& directory() const { return directoryName_; }
    uint32_t cellCount() const { return uint32_t(toc_.objectCount() - 1); }

    // ExpressionMatrixSubset (src/ExpressionMatrixSubset.cpp:9-42): CSR restricted to the gene set and the
    // cell set, in local ids.  Throws the reference's "Gene set X does not exist." etc.
    void subset(const std::string& geneSetName, const std::string& cellSetName, std::vector<uint64_t>& toc,
                std::vector<em2_count>& data, uint32_t& geneCount, uint32_t& cellCount) const;

    // The lookups and checks of subset() without building it; runLshPath builds it on the device.
    void lookupSubset(const std::string& geneSetName, const std::string& cellSetName, const GeneSet*& genes,
                      const uint32_t*& cellIds, uint32_t& cellCount) const;
    // pairsFor(cellCount) returns where the pairs are to be written (used != nullptr asks for pairs at all).
    void runLshPath(const char* what, const std::string& geneSetName, const std::string& cellSetName, size_t lshCount,
                    unsigned int seed, uint32_t& cellCount, std::vector<uint64_t>* signatures, size_t k,
                    double similarityThreshold, const std::function<em2_pair*(uint32_t)>& pairsFor,
                    std::vector<uint32_t>* used) const;

    void findSimilarPairs4(const std::string& geneSetName, const std::string& cellSetName,
                           const std::string& similarPairsName, size_t k, double similarityThreshold,
                           size_t lshCount, unsigned int seed) const;
    void computeLshSignatures(const std::string& geneSetName, const std::string& cellSetName,
                              const std::string& lshName, size_t lshCount, unsigned int seed) const;
    void findSimilarPairs5(const std::string& geneSetName, const std::string& cellSetName,
                           const std::string& lshName, const std::string& similarPairsName, size_t k,
                           double similarityThreshold, size_t lshSliceLength, size_t bucketOverflow) const;
    void findSimilarPairs6(const std::string& geneSetName, const std::string& cellSetName, const std::string& lshName,
                           const std::string& similarPairsName, size_t k, double similarityThreshold, size_t permutationCount,
                           size_t searchCount, size_t permutedBitCount, int seed) const;
    void findSimilarPairs7(const std::string& geneSetName, const std::string& cellSetName, const std::string& lshName,
                           const std::string& similarPairsName, size_t k, double similarityThreshold,
                           const std::vector<int32_t>& lshSliceLengths, uint32_t maxCheck, size_t log2BucketCount) const;
    void removeSimilarPairs(const std::string& similarPairsName) const;
    // ExpressionMatrix::findSimilarPairs0 (src/ExpressionMatrixFindSimilarPairs.cpp:16-99): exact, all pairs.
    void findSimilarPairs0(const std::string& geneSetName, const std::string& cellSetName, const std::string& similarPairsName,
                           size_t k, double similarityThreshold) const;
    // ExpressionMatrix::findSimilarGenePairs0 (src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198) without its csv, and
    // removeSimilarGenePairs (:223-232).
    void findSimilarGenePairs0(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod,
                               const std::string& similarGenePairsName, size_t k, double similarityThreshold) const;
    void removeSimilarGenePairs(const std::string& similarGenePairsName) const;
    // ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150): writes <name>-analysis.csv and
    // <name>-analysis-statistics.csv into outputDirectory (the reference: the working directory, "").
    void analyzeSimilarPairs(const std::string& similarPairsName, double csvDownsample, const std::string& outputDirectory) const;
    // ExpressionMatrix::computeCellSimilarity (src/ExpressionMatrix.cpp:1456-1537): global cell ids, one pair, on the host.
    double computeCellSimilarity(const std::string& geneSetName, uint32_t cellId0, uint32_t cellId1) const;
    // The two colourings of the cell graph that are numbers per cell (src/ExpressionMatrixHttpServerGraphs.cpp:788-850), on the
    // device: computeCellSimilarity of cellId0 against every cell of a list (em2_cell_similarities_to_cell), and the value
    // computeExpressionVector gives one gene in every cell of a list (em2_gene_expression_of_cells).  Global ids; only the rows
    // the call needs go to the device.  A gene outside the gene set is the reference's CZI_ASSERT (:821), EM2_ERROR_RUNTIME.
    void cellSimilaritiesToCell(const std::string& geneSetName, uint32_t cellId0, const uint32_t* cellIds, uint32_t count, double* out) const;
    void geneExpressionOfCells(const std::string& geneSetName, uint32_t globalGeneId, int normalizationMethod, const uint32_t* cellIds,
                               uint32_t count, float* out) const;
    // ExpressionMatrix::compareSimilarPairs (src/ExpressionMatrixLsh.cpp:1199-1240): writes CompareSimilarPairs.csv.
    void compareSimilarPairs(const std::string& similarPairsName0, const std::string& similarPairsName1,
                             const std::string& outputDirectory) const;
    // ExpressionMatrix::analyzeLsh (src/ExpressionMatrixLsh.cpp:1244-1367): writes Lsh-analysis.csv and
    // LSH-analysis-statistics.csv into outputDirectory (the reference: the working directory, "").
    void analyzeLsh(const std::string& geneSetName, const std::string& cellSetName, size_t lshCount, unsigned int seed,
                    double csvDownsample, const std::string& outputDirectory) const;

    // ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150) without its name bookkeeping: the
    // lookups and their errors, then em2_signature_graph_create on the signatures of Lsh-<lshName>.  The caller frees *graph.
    void createSignatureGraph(const std::string& cellSetName, const std::string& lshName, uint64_t minCellCount,
                              em2_signature_graph** graph) const;
    // ExpressionMatrix::analyzeLshSignatures (src/ExpressionMatrixLsh.cpp:1372-1474): writes Signatures.csv, Histogram.csv and
    // LshSignatureStatistics.csv into outputDirectory (the reference: the working directory, "").
    void analyzeLshSignatures(const std::string& geneSetName, const std::string& cellSetName, size_t lshCount, unsigned int seed,
                              const std::string& outputDirectory) const;

    // ExpressionMatrix::createGeneGraph (src/ExpressionMatrixGeneGraph.cpp:54-89) without its name bookkeeping: the lookups and
    // their errors, then em2_gene_graph_create on SimilarGenePairs-<similarGenePairsName>.  k is the reference's int, which the
    // GeneGraph constructor takes as a size_t.  The caller frees *graph.
    void createGeneGraph(const std::string& geneSetName, const std::string& similarGenePairsName, int64_t k, double similarityThreshold,
                         em2_gene_graph** graph) const;
    // createGeneSetIntersection / createGeneSetUnion (src/ExpressionMatrixGeneSets.cpp:183-250) and createGeneSetDifference
    // (:254-305).  false and `message` = the line the reference prints where it returns false; it does not throw for these.
    bool createGeneSetIntersectionOrUnion(const std::string& commaSeparatedInputSetsNames, const std::string& outputSetName, bool doUnion,
                                          std::string& message);
    bool createGeneSetDifference(const std::string& inputSetName0, const std::string& inputSetName1, const std::string& outputSetName,
                                 std::string& message);

    // ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) for the genes of a gene set over a
    // cell set, and the cells expressing every gene (src/ExpressionMatrixGeneSets.cpp:336-350); either vector may be NULL.
    // The cells' norm inverses come from the Cells file where the directory has one.
    void geneInformation(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod,
                         std::vector<float>* informationContent, std::vector<uint32_t>* expressingCellCount) const;
    // em2_matrix_rank_genes: the rank-sum integers and statistics of the genes of a gene set for groups of the
    // cells of a cell set; group[size of the cell set], a cell with EM2_GROUP_EXCLUDED is left out.  Outputs [genes][groupCount]
    // (groupSize [groupCount], tieSum [genes]); zScore and auc may be NULL.
    void rankGenes(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod, const uint32_t* group,
                   uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2, uint64_t* tieSum, double* zScore,
                   double* auc) const;
    // createGeneSetUsingInformationContent (src/ExpressionMatrix.cpp:2022-2082), createWellExpressedGeneSet
    // (src/ExpressionMatrixGeneSets.cpp:314-362) and removeGeneSet (:12-32): the new set's files, and the set under its name.
    void createGeneSetUsingInformationContent(const std::string& existingGeneSetName, const std::string& cellSetName,
                                              int normalizationMethod, double geneInformationContentThreshold,
                                              const std::string& newGeneSetName);
    void createWellExpressedGeneSet(const std::string& inputGeneSetName, const std::string& inputCellSetName,
                                    const std::string& outputGeneSetName, uint32_t minCellCount);
    void removeGeneSet(const std::string& geneSetName);

    // createCellSet (src/ExpressionMatrix.cpp:1626-1633, CellSets::addCellSet src/CellSets.cpp:65-83),
    // createCellSetIntersection / Union (:1642-1696), createCellSetDifference (:1700-1737), downsampleCellSet (:1742-1777) and
    // removeCellSet (src/CellSets.cpp:88-97).  These throw in the reference and here; include/em2_lsh.h states the departures.
    void createCellSet(const std::string& cellSetName, std::vector<uint32_t> cellIds);
    void createCellSetIntersectionOrUnion(const std::string& commaSeparatedInputSetsNames, const std::string& outputSetName, bool doUnion);
    void createCellSetDifference(const std::string& inputSetName0, const std::string& inputSetName1, const std::string& outputSetName);
    void downsampleCellSet(const std::string& inputCellSetName, const std::string& outputCellSetName, double probability, int seed);
    void removeCellSet(const std::string& cellSetName);
    std::vector<std::string> cellSetNames() const;           // std::map order

    // getDenseExpressionMatrix (src/PythonModule.cpp:78-154): the checks in the reference's order, then the rows
    // [rowBegin, rowEnd) of the cell set, with their global gene ids, through em2_dense_expression into out.
    void denseExpression(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod, int elementType,
                         uint32_t rowBegin, uint32_t rowEnd, void* out) const;
    // The stored entries of a cell (getCellExpressionCounts, src/ExpressionMatrix.cpp:1066-1075) in the mapped file.
    void cellExpressionCounts(uint32_t cellId, const em2_count*& entries, uint64_t& count) const;

    // Cell meta data (em2_meta_data.cpp; the store's formats are in em2_meta_data.h).  The store is read when the directory is
    // opened -- a directory without the CellMetaData* files is one where no cell has a field -- kept in host memory, created
    // by the first write and written back by flush() and by the destructor.
    //   setCellMetaData             src/ExpressionMatrix.cpp:942-967; cellMetaDataValue / cellMetaData :880-922;
    //   removeCellMetaData          :998-1029; createCellSetUsingMetaData :1560-1622;
    //   metaDataTable               histogramMetaData (:1301-1323) of one field (metaDataName1 == NULL) or two and the
    //                               contingency table of :1369-1381, through em2_contingency_create;
    //   computeMetaDataRandIndex    :1328-1390.
    void setCellMetaData(uint32_t cellId, const std::string& name, const std::string& value);
    std::string cellMetaDataValue(uint32_t cellId, const std::string& name) const;
    std::vector<std::pair<std::string, std::string>> cellMetaData(uint32_t cellId) const;
    void removeCellMetaData(const std::string& cellSetName, const std::string& metaDataName);
    void createCellSetUsingMetaData(const std::string& cellSetName, const std::string& metaDataFieldName, const std::string& matchString,
                                    bool useRegex);
    void metaDataTable(const std::string& cellSetName, const std::string& metaDataName0, const std::string* metaDataName1,
                       MetaDataTable& out) const;
    void computeMetaDataRandIndex(const std::string& cellSetName, const std::string& metaDataName0, const std::string& metaDataName1,
                                  double& randIndex, double& adjustedRandIndex) const;
    // colorByMetaDataInterpretedAsCategory (src/ExpressionMatrixSignatureGraph.cpp:198-264) for vertices that hold ids into
    // globalCellIds (em2_pie_host.cpp; include/em2_lsh.h says what runs where).  The caller frees *census.
    void pieCensus(uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                   const uint32_t* globalCellIds, uint32_t cellSetSize, const std::string& metaDataName, em2_pie_census** census) const;
    void flush();

    // Ingest (em2_ingest_host.cpp; the files are in em2_ingest.h).  create is ExpressionMatrix::createNew
    // (src/ExpressionMatrix.cpp:56-101): an error if the directory exists; the matrix it returns is open.  The methods that
    // need the files only create() writes throw EM2_ERROR_RUNTIME with the missing file's name on a directory without them.
    //   addGene                     src/ExpressionMatrixGenes.cpp:12-39
    //   geneName, geneIdFromName, cellIdFromString    src/ExpressionMatrix.cpp:822-874 (0xffffffff = not found)
    //   addCell                     :165-294; a failing call leaves the store as it was
    //   addCellsFromCsr             the per-barcode loop of addCellsFromHdf5 (src/ExpressionMatrixHdf5.cpp:113-200) on the
    //                               arrays of the file, the cells' entries on the device; all or nothing, the error of the
    //                               lowest failing barcode.  skip[i] != 0: the barcode is below the count threshold.
    static Matrix* create(const std::string& directoryName);
    uint32_t geneCount() const;
    bool addGene(const std::string& geneName);
    std::string geneName(uint32_t geneId) const;
    uint32_t geneIdFromName(const std::string& geneName) const;
    uint32_t cellIdFromString(const std::string& s) const;
    uint32_t addCell(const std::vector<std::pair<std::string, std::string>>& metaData,
                     const std::vector<std::pair<std::string, float>>& expressionCounts);
    void addCellsFromCsr(const std::vector<std::string>& geneNames, const std::vector<std::string>& cellNames, const uint64_t* indptr,
                         const uint32_t* indices, const float* values, uint64_t entryCount, const uint8_t* skip,
                         const std::string& cellNamePrefix, const std::vector<std::pair<std::string, std::string>>& cellMetaData,
                         uint64_t chunkBytes, uint32_t& firstCellId, uint32_t& addedCellCount);
    // The files of the reference's own workflow (em2_csv_host.cpp, em2_csv.hip; the rules are in include/em2_lsh.h).
    //   addCellsFromCsv             addCells, src/ExpressionMatrix.cpp:380-654; all or nothing.  useDevice == false: the host
    //                               path.  *deferredFieldCount (may be NULL): the fields the device handed to the host.
    //   addCellMetaDataFromFile     addCellMetaData, src/ExpressionMatrixBioHub.cpp:337-392; host only, all or nothing.
    void addCellsFromCsv(const std::string& expressionCountsFileName, const std::string& expressionCountsFileSeparators,
                         const std::string& cellMetaDataFileName, const std::string& cellMetaDataFileSeparators,
                         const std::vector<std::pair<std::string, std::string>>& additionalCellMetaData, uint64_t chunkBytes,
                         bool useDevice, uint32_t& firstCellId, uint32_t& addedCellCount, uint64_t* deferredFieldCount);
    void addCellMetaDataFromFile(const std::string& cellMetaDataFileName);

    const GeneSet& geneSet(const std::string& name) const;                 // throws "Gene set X does not exist."
    const MappedFile& cellSet(const std::string& name) const;              // throws "Cell set X does not exist."

private:
    // The rows of `cellIds`, then the rows of `more`, as a CSR of their own with the global gene ids.
    void gatherRows(const char* who, const uint32_t* cellIds, uint32_t count, const std::vector<uint32_t>& more, std::vector<uint64_t>& toc,
                    std::vector<em2_count>& data) const;
    // The norm1Inverse (method 1) or norm2Inverse (method 2) of these cells from the Cells file; empty where the directory has none.
    std::vector<double> normInversesFromFile(const uint32_t* cellIds, uint32_t count, int normalizationMethod) const;
    // Writes GeneSet-<name>-* for the genes of `from` that `keep` names (ascending local id) and opens the new set.
    void addGeneSubset(const std::string& name, const GeneSet& from, const std::vector<bool>& keep);
    // The same for ascending global ids.
    void addGeneSetOf(const std::string& name, const std::vector<uint32_t>& ids);
    bool knowsGeneSet(const std::string& name) const;
    void failIfGeneSetExists(const std::string& name) const;
    // CellSets::exists for the sets this object knows and, as knowsGeneSet, a file another object has written since.
    bool knowsCellSet(const std::string& name) const;
    void failIfCellSetExists(const std::string& name) const;
    // CellSets::addCellSet: sorts and deduplicates, writes CellSet-<name> and opens it under its name.
    void addCellSetOf(const std::string& name, std::vector<uint32_t>& ids);
    std::string directoryName_;
    MappedFile toc_;         // CellExpressionCounts.toc  (uint64)
    MappedFile data_;        // CellExpressionCounts.data (em2_count)
    std::map<std::string, GeneSet*> geneSets_;
    std::map<std::string, MappedFile*> cellSets_;
    void openMetaData();
    void closeMetaData();
    void checkCellId(const char* who, uint32_t cellId) const;
    const MappedFile& cellSetForMetaData(const std::string& cellSetName) const;    // throws "Cell set X not found."
    MetaDataStore* metaData_;
    void openIngest(bool writable);
    void closeIngest();
    void flushIngest();
    IngestState& ingest(const char* who) const;               // throws where the directory is no complete store
    // The writes of addCell after its checks: the name, the meta data list, the entries, the Cell record, AllCells.
    void commitCell(const std::vector<std::pair<std::string, std::string>>& metaData, const em2_count* entries, uint64_t entryCount,
                    const void* cellRecord);
    // The writing half of a bulk add: the new genes in order, then cell i of [0, cellCount) with the list metaDataOf(i) gives
    // (CellName first; NULL: the cell is skipped), its entries data[toc[i], toc[i + 1]) and its 56-byte record.  String ids
    // come out in the reference's order of first insertion.  Returns the number of cells written.
    uint32_t writeCells(const std::vector<std::string>& newGenes, size_t cellCount,
                        const std::function<const std::vector<std::pair<std::string, std::string>>*(size_t)>& metaDataOf,
                        const uint64_t* toc, const em2_count* data, const void* cellRecords);
    IngestState* ingest_;
};

// SimilarPairs files (src/SimilarPairs.cpp:11-42 create, :369-379 copy): -Info, -Pairs, -CellInfo.
// SimilarPairs(directory, name, geneSetName, cellSetName, k) for writing (src/SimilarPairs.cpp:11-42): creates the three
// files; the pairs are written in place (k per cell, the caller's order is final), finish() fills CellInfo.
class SimilarPairsWriter {
public:
    SimilarPairsWriter(const std::string& directoryName, const std::string& similarPairsName, const std::string& geneSetName,
                       const std::string& cellSetName, size_t k, uint32_t cellCount);
    ~SimilarPairsWriter();                    // not finished: the temporary files go away, an existing object stays
    em2_pair* pairs();
    // fills CellInfo, then renames the three files into place.  Without the two lowest* arrays CellInfo keeps the
    // constructor's values, as after SimilarPairs::copy; with them it holds what SimilarPairs::add left (findSimilarPairs0).
    void finish(const uint32_t* usedCount, const uint32_t* lowestSimilarityIndex = nullptr, const float* lowestSimilarity = nullptr);
private:
    void removeStale() const;
    MappedFile infoFile_, pairsFile_, cellInfoFile_;
    uint32_t cellCount_;
    std::string base_;
    bool finished_;
};

void writeSimilarPairs(const std::string& directoryName, const std::string& similarPairsName,
                       const std::string& geneSetName, const std::string& cellSetName, size_t k,
                       uint32_t cellCount, const em2_pair* pairs, const uint32_t* usedCount);

struct SimilarPairsInfo {
    uint64_t k;
    std::string geneSetName;
    uint64_t geneSetHash;
    std::string cellSetName;
    uint64_t cellSetHash;
    uint64_t cellCount;
};
// Existing-object constructor of SimilarPairs (src/SimilarPairs.cpp:47-83) including its consistency checks.
void readSimilarPairs(const std::string& directoryName, const std::string& similarPairsName,
                      SimilarPairsInfo& info, std::vector<em2_pair>* pairs, std::vector<uint32_t>* usedCount);

// SimilarGenePairs files (src/SimilarGenePairs.cpp:8-48 create, :53-89 access): -Info, -Pairs (k slots per gene of the gene set,
// local gene ids), -GeneInfo (usedCount).  The write takes pairs that are already selected and sorted.
struct SimilarGenePairsInfo {
    uint64_t k;
    std::string geneSetName;
    uint64_t geneSetHash;
    std::string cellSetName;
    uint64_t cellSetHash;
    int32_t normalizationMethod;          // NormalizationMethod (src/NormalizationMethod.hpp:11-16): 0 none, 1 L1, 2 L2
    uint64_t geneCount;
};
void writeSimilarGenePairs(const std::string& directoryName, const std::string& similarGenePairsName, const std::string& geneSetName,
                           const std::string& cellSetName, size_t k, int normalizationMethod, uint32_t geneCount,
                           const em2_pair* pairs, const uint32_t* usedCount);
void readSimilarGenePairs(const std::string& directoryName, const std::string& similarGenePairsName, SimilarGenePairsInfo& info,
                          std::vector<em2_pair>* pairs, std::vector<uint32_t>* usedCount);
// The last step of findSimilarGenePairs0 (:186): std::sort of every gene's usedCount[g] pairs by similarity alone, descending
// -- this library's libstdc++ introsort on the arrangement the selection left, as in the reference.
void sortGenePairs(em2_pair* pairs, const uint32_t* usedCount, uint32_t geneCount, size_t k);

// Lsh files (src/Lsh.hpp:136-141, src/Lsh.cpp:26-28,148): <prefix>-Info, <prefix>-Signatures.
void writeLsh(const std::string& prefix, uint64_t cellCount, uint64_t lshCount, const uint64_t* signatures);
void readLshInfo(const std::string& prefix, uint64_t& cellCount, uint64_t& lshCount);
void readLsh(const std::string& prefix, uint64_t& cellCount, uint64_t& lshCount, std::vector<uint64_t>& signatures);

// Test / bench tooling (NOT a reference API): a directory holding exactly the files the LSH path reads.
void createDirectoryFromCsr(const std::string& directoryName, uint32_t geneCount, uint32_t cellCount,
                            const uint64_t* toc, const em2_count* data);
void addGeneSet(const std::string& directoryName, const std::string& name, const uint32_t* sortedGlobalIds,
                uint32_t count, uint32_t totalGeneCount);
void addCellSet(const std::string& directoryName, const std::string& name, const uint32_t* sortedCellIds,
                uint32_t count);
// A Cells file (MemoryMapped::Vector<Cell>, src/Cell.hpp) holding these inverses, zeros elsewhere.
void addCells(const std::string& directoryName, const double* norm1Inverse, const double* norm2Inverse, uint32_t cellCount);

}  // namespace host
}  // namespace em2

#endif
