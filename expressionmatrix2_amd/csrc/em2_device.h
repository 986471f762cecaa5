// em2_device.h -- internal declarations shared by the HIP translation units and the C ABI glue.
#ifndef EM2_DEVICE_H
#define EM2_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "em2_select.h"

namespace em2 {

// Layout-compatible with std::pair<CellId, float> (src/SimilarPairs.hpp:53-56) and em2_pair (include/em2_lsh.h).
struct PairOut {
    uint32_t cell;
    float similarity;
};

// Layout-compatible with std::pair<GeneId, float> (src/ExpressionMatrixSubset.hpp:36) and em2_count.
struct CountIn {
    uint32_t gene;
    float count;
};

// Device-resident copies of the tables of em2_tables.h.
struct DeviceTables {
    const uint32_t* keyOfMismatch;   // [lshCount+1]
    const int32_t* acceptMaxByKey;   // [keyCount]
    const float* keySimilarity;      // [keyCount]
    int32_t mGlobal;
    int32_t mMaxInitial;
    bool identityKeys;               // keyOfMismatch[m] == m for every m
};

// Signature words per cell padded to a supported kernel width (in 32-bit words); 0 if lshCount is too large.
uint32_t paddedDwords(uint32_t lshCount);

// Copies [cellCount][wordCount] uint64 signatures into the zero-padded [cellCount][paddedDwords/2] layout.
hipError_t launchRepackSignatures(const uint64_t* src, uint32_t cellCount, uint32_t wordCount,
                                  uint32_t* dst, uint32_t paddedDw, hipStream_t stream);

// Largest k the scan kernel supports (limited by the per-wave LDS staging area).
uint32_t fsp4MaxK();

// findSimilarPairs4 for rows [rowBegin,rowEnd) against all cellCount columns.
//   sig32    [cellCount][paddedDw] device
//   buffers  [(rowEnd-rowBegin)][2k] Entry, device scratch
//   outPairs [(rowEnd-rowBegin)][k], outUsed [(rowEnd-rowBegin)]
//   control  fsp4ControlBytes(rows) bytes of device scratch for the persistent kernel's hand-off state (NULL
//            selects the simple one-wave-per-row-block kernel)
hipError_t launchFsp4Scan(const uint32_t* sig32, uint32_t paddedDw, uint32_t cellCount,
                          uint32_t rowBegin, uint32_t rowEnd, uint32_t k, const DeviceTables& tables,
                          Entry* buffers, PairOut* outPairs, uint32_t* outUsed, void* control,
                          hipStream_t stream, void* symmetricWorkspace = nullptr);
size_t fsp4ControlBytes(uint32_t rowCount);
// Extra scratch for the symmetric (each unordered pair once) form of the scan, which launchFsp4Scan uses when all
// rows of the problem are in one launch and this workspace is given; 0 when that form would not be used.
size_t fsp4SymmetricBytes(uint32_t cellCount, uint32_t rowCount, uint32_t paddedDw);
bool fsp4UsesSymmetricScan(uint32_t cellCount, uint32_t rowCount, uint32_t paddedDw);
// Whether a launch of rowCount rows against cellCount columns that is not symmetric takes the rows form on the matrix
// cores (form 4: every row walks all columns as FP4 dot products); fsp4SymmetricBytes then sizes its workspace.
bool fsp4UsesRowsMatrixScan(uint32_t cellCount, uint32_t rowCount, uint32_t paddedDw);
// Whether signatures of this padded width take the matrix-core form of the symmetric scan (EM2_SCAN_MATRIX included).
bool fsp4MatrixFormWanted(uint32_t paddedDw);
struct Fsp4LaunchInfo {
    int form;                 // 0 ordered rows x columns, 1 symmetric, 2 sharded symmetric, 3 symmetric on the matrix cores, 4 rows x columns on the matrix cores
    double scanKernelMs;      // duration of the scan kernel proper when the launcher measured it (symmetric form), else -1
    double waveColumnSteps;   // (64-row wave, column) steps executed: x 64 lanes x 2*W32 = v_xor/v_bcnt lane-ops
    double inboxEntries;      // symmetric form: entries (incl. chunk padding) sorted and replayed
    double segments;
    double fullRowCells;
    double matrixPairs;       // form 3: (row, column) pairs contracted on the matrix cores
    double matrixKernelMs;    // form 3: duration of fsp4ScanMatrixKernel alone
    double matrixClockGHz;    // form 3: the shader clock that kernel ran at (block-lifetime s_memtime / s_memrealtime sums), 0 if unknown
};
Fsp4LaunchInfo fsp4LastLaunchInfo();      // of the calling thread's last launchFsp4Scan
hipError_t readFsp4Error(const void* control, uint32_t rowCount, hipStream_t stream, uint32_t* error);

// Sharded symmetric scan (em2_scan.hip): plan of one rank, one launch per phase; the collectives between the phases
// belong to the caller.
struct Fsp4ShardPlan {
    bool eligible;
    uint32_t cellCount, world, rank, k;
    uint32_t blocks, prefixBlocks, prefixCells, ownBlocks, maxOwnBlocks, ownPrefixBlocks;
    uint64_t capLocal, capGathered;
    size_t sortTempBytes;
    size_t offLists, offControl, offSnap, offTable, offInboxControl, offPool, offFragments, offTerms, rankBytes, offGathered, offSorted, offTemp, totalBytes;
};
Fsp4ShardPlan fsp4ShardPlan(uint32_t cellCount, uint32_t k, uint32_t rank, uint32_t world);
hipError_t launchFsp4ShardPhase(const Fsp4ShardPlan& plan, int phase, const uint32_t* sig32, uint32_t paddedDw,
                                const DeviceTables& tables, void* rankWs, void* exchangeWs, PairOut* outPairs,
                                uint32_t* outUsed, uint64_t gatheredCount, hipStream_t stream);
hipError_t readFsp4ShardStatus(const Fsp4ShardPlan& plan, const void* rankWs, hipStream_t stream, uint64_t* used,
                               uint32_t* overflow, uint32_t* error);

// ExpressionMatrixSubset::computeSums (sum1 only) -> mean = sum1 / geneCount, per cell.
hipError_t launchCellMeans(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount,
                           double* means, hipStream_t stream);

// lshVectorsSums[i] = sum over genes (ascending) of vectors[g][i]   (Lsh.cpp:137-144)
hipError_t launchVectorSums(const double* vectors, uint32_t geneCount, uint32_t lshCount, double* sums,
                            hipStream_t stream);

// Lsh::computeCellLshSignatures for the cellCount cells of the CSR (toc[0..cellCount], data); writes
// signatures[cellCount][wordCount].  means[cellCount] from launchCellMeans.
hipError_t launchProjection(const uint64_t* toc, const CountIn* data, uint32_t cellCount, const double* vectors,
                            const double* vectorSums, const double* means, uint32_t lshCount,
                            uint64_t* signatures, hipStream_t stream);

// Screened projection (em2_project.hip): aux = per-bit sums and max |U|, and a float copy of the hyperplanes,
// built once per hyperplane matrix; requires lshCount % 4 == 0.  Result identical to launchProjection.
size_t vectorAuxBytes(uint32_t geneCount, uint32_t lshCount);
hipError_t launchPrepareVectors(const double* vectors, uint32_t geneCount, uint32_t lshCount, void* aux,
                                hipStream_t stream);
size_t projectionScreenedWorkspaceBytes(uint32_t cellCount, uint32_t lshCount);
hipError_t launchProjectionScreened(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount,
                                    const double* vectors, const void* aux, uint32_t lshCount, uint64_t* signatures,
                                    void* workspace, hipStream_t stream);

// findSimilarPairs5 (src/ExpressionMatrixLsh.cpp:355-496): bucket tables over all cells, results for the cells
// [rowBegin,rowEnd).  Allocates its own scratch (from the cache of em2_scratch.h) and synchronises the stream.  q = lshSliceLength in [1,32].
// What the calling thread's last runFsp5 did (benchmarks): candidate ids gathered from the buckets (duplicates and the
// cell itself included), cells queried, slices, batches, and the HIP-event durations of the candidate filter (the
// gather of candidate signatures + popcounts) and of the selection over all batches.
struct Fsp5LaunchInfo {
    double gatheredCandidates, cells, sliceCount, batches, filterMs, selectMs;
    double distinctCandidates;      // what the filter read: the sizes of the cells' duplicate-free unions (the cell itself included); -1 in the sort form
    // which forms ran (host-side facts; tests assert the path they mean to exercise through them)
    double unionForm;               // 1 = bitmap in LDS (unionKernel), 0 = gatherKernel + segmented sort
    double unionPasses;             // passes of the bitmap over the id range, ceil(cellCount / unionIdsPerPass); 0 in the sort form
    double unionIdsPerPass;         // cell ids one pass of the bitmap covers
    double filterForm;              // Fsp5FilterForm
    double selectPacked;            // 1 = selectPackedKernel tiers ({key, position} in 4 bytes), 0 = selectKernel tiers of whole entries
};
// The candidate filter by shape (runFsp5); the wide forms are filterWideKernel<T, LPC, FULL>.
enum Fsp5FilterForm {
    kFsp5FilterLane = 0,            // filterKernel: one lane per candidate
    kFsp5FilterCooperative = 1,     // filterCooperativeKernel
    kFsp5FilterWide_4_4_full = 2,
    kFsp5FilterWide_1_16 = 3,
    kFsp5FilterWide_1_8 = 4,
    kFsp5FilterWide_1_0 = 5,
    kFsp5FilterWide_2_16_full = 6,
    kFsp5FilterWide_2_16 = 7,
    kFsp5FilterWide_2_0 = 8
};
Fsp5LaunchInfo fsp5LastLaunchInfo();
void fsp4SetInboxEntriesPerCell(uint32_t entries);       // (this thread's symmetric scans: 0 = the default of 1024; em2_scan_symmetric.hip)

hipError_t runFsp5(const uint64_t* d_sig, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t lshCount,
                   uint32_t k, uint32_t q, uint64_t bucketOverflow, const DeviceTables& tables, PairOut* d_pairs,
                   uint32_t* d_used, hipStream_t stream);

// ExpressionMatrixSubset::ExpressionMatrixSubset (src/ExpressionMatrixSubset.cpp:9-42) on the device (em2_subset.hip).
// cellIds == NULL means all cells in order; geneLocalIds[globalGeneId] = local id or 0xffffffff.
size_t subsetWorkspaceBytes(uint32_t cellCount);
hipError_t launchSubsetCount(const uint64_t* globalToc, const CountIn* globalData, const uint32_t* cellIds, uint32_t cellCount,
                             const uint32_t* geneLocalIds, uint32_t globalGeneCount, uint64_t* toc, void* workspace,
                             size_t workspaceBytes, hipStream_t stream);
hipError_t launchSubsetFill(const uint64_t* globalToc, const CountIn* globalData, const uint32_t* cellIds, uint32_t cellCount,
                            const uint32_t* geneLocalIds, uint32_t globalGeneCount, const uint64_t* toc, CountIn* outData,
                            hipStream_t stream);

// findSimilarPairs7 (src/ExpressionMatrixLsh.cpp:507-827), results for the cells [rowBegin,rowEnd).  Allocates its own
// scratch and synchronises the stream.
uint32_t fsp7MaxK();
hipError_t runFsp7(const uint64_t* d_sig, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t lshCount, uint32_t k,
                   const int32_t* sliceLengths, uint32_t sliceLengthCount, uint32_t maxCheck, uint32_t log2BucketCount,
                   uint64_t mismatchThreshold, const DeviceTables& tables, PairOut* d_pairs, uint32_t* d_used, hipStream_t stream);

// findSimilarPairs6 (src/ExpressionMatrixLsh.cpp:842-1145), results for the cells [rowBegin,rowEnd); the sorted tables
// always cover all cells.  Allocates its own scratch and synchronises the stream.  The limits are those of the kernels'
// LDS: permutationCount, fsp6EffectiveSearch() (searchCount capped by what the queue can hold) and permutedBitCount.
uint32_t fsp6MaxPermutations();
uint32_t fsp6MaxSearch();
uint32_t fsp6MaxPermutedBits();
uint64_t fsp6EffectiveSearch(uint32_t cellCount, uint32_t permutationCount, uint32_t searchCount);
hipError_t runFsp6(const uint64_t* d_sig, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd, uint32_t lshCount, uint32_t k,
                   uint32_t permutationCount, uint32_t searchCount, uint32_t permutedBitCount, int32_t seed,
                   const DeviceTables& tables, PairOut* d_pairs, uint32_t* d_used, hipStream_t stream);

// CellGraph::CellGraph (src/CellGraph.cpp:33-117): edges of the k-NN graph in the reference's insertion order.
hipError_t runCellGraphEdges(const PairOut* pairs, const uint32_t* usedCount, uint32_t spCellCount, uint32_t k,
                             const uint32_t* spCellSet, const uint32_t* graphCellSet, const uint32_t* graphSortedIds,
                             const uint32_t* graphVertexOfSorted, uint32_t graphCellCount, double similarityThreshold,
                             uint32_t maxConnectivity, uint32_t* edge0, uint32_t* edge1, float* edgeSimilarity,
                             uint64_t* edgeCountHost, hipStream_t stream, bool spConsecutive, uint32_t spFirst, bool graphConsecutive,
                             uint32_t graphFirst);

// CellGraph::labelPropagationClustering (src/CellGraph.cpp:443-612) on the device (em2_cluster.hip).  Host buffers;
// labels[v] = the raw label (a cell id) of vertex v after the last iteration.
hipError_t runLabelPropagation(const uint32_t* vertexCellIds, uint32_t vertexCount, const uint32_t* edgeVertex0,
                               const uint32_t* edgeVertex1, const float* edgeSimilarity, uint64_t edgeCount,
                               const uint32_t* shuffleInput, uint64_t seed, uint64_t stableIterationCountThreshold,
                               uint64_t maxIterationCount, uint32_t* labels, uint64_t* iterationCount, uint32_t* error,
                               hipStream_t stream);

// em2_analyze.hip: ExpressionMatrix::analyzeLsh (src/ExpressionMatrixLsh.cpp:1244-1367).  Device half: per unordered pair
// of rows [rowBegin, rowEnd) x the cells above each, the sparse scalar product of the two cells' counts (float products,
// double sum, ascending gene order) and the mismatch count of their signatures.  Host half: the order-defined rest.
uint64_t analyzePairCount(uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd);
size_t analyzeScratchBytes(uint32_t geneCount, uint32_t rowCount);
hipError_t launchAnalyzePairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount,
                              const uint64_t* signatures, uint32_t words, uint32_t rowBegin, uint32_t rowEnd, void* scratch,
                              double* scalarProducts, uint32_t* mismatches, hipStream_t stream);
// The host half of ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150) takes the same three steps
// over the exact similarities launchStoredPairs gives.  Begin returns NULL where the csv cannot be opened; Rows returns false
// where the reference's bin assert throws; analysisEnd (lshCount 0 after analyzeStoredBegin) writes the statistics csv,
// returns false where it cannot be opened, and deletes the state.
struct AnalysisState;
AnalysisState* analyzeLshBegin(uint32_t lshCount, uint32_t seed, const char* pairsCsvPath);
bool analyzeLshRows(AnalysisState* s, const double* sums, uint32_t cellCount, uint32_t geneCount, const uint32_t* globalCellIds,
                    uint32_t rowBegin, uint32_t rowEnd, const double* scalarProducts, const uint32_t* mismatches, double csvDownsample,
                    double* exactOut, double* lshOut);
AnalysisState* analyzeStoredBegin(const char* pairsCsvPath);
bool analyzeStoredRows(AnalysisState* s, const PairOut* pairs, const uint32_t* usedCount, uint32_t k, const uint32_t* globalCellIds,
                       uint32_t rowBegin, uint32_t rowEnd, const double* exact, double csvDownsample);
bool analysisEnd(AnalysisState* s, uint32_t lshCount, const char* statisticsCsvPath, uint64_t* sum0, double* sum1, double* sum2);

// em2_fsp0.hip: ExpressionMatrix::findSimilarPairs0 (src/ExpressionMatrixFindSimilarPairs.cpp:16-99) for the cells
// [rowBegin,rowEnd) against all cells: exact similarities, SimilarPairs::add replayed per cell, the lists sorted.  The
// slots of a cell live in LDS: min(k, cellCount - 1) <= fsp0MaxSlots().  workspace: fsp0WorkspaceBytes().  Synchronises
// the stream.  *inputError != 0: a gene id not below geneCount (bit 0) or not ascending within a cell (bit 1).
uint32_t fsp0MaxSlots();
bool fsp0Supported(uint32_t cellCount, uint32_t k);
size_t fsp0WorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, uint32_t k);
hipError_t runFsp0(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin, uint32_t rowEnd,
                   uint32_t k, double similarityThreshold, PairOut* outPairs, uint32_t* outUsed, uint32_t* outLowestIndex,
                   float* outLowestSimilarity, void* workspace, uint32_t* inputError, hipStream_t stream);
// The device half of ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150): the exact similarity of
// every stored pair of the rows, exact[(row - rowBegin) * k + t].  prepareStoredPairs fills the workspace once.
size_t storedPairsWorkspaceBytes(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount);
hipError_t prepareStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, void* workspace,
                              uint32_t* inputError, hipStream_t stream);
hipError_t launchStoredPairs(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, uint32_t rowBegin,
                             uint32_t rowEnd, const PairOut* pairs, const uint32_t* usedCount, uint32_t k, void* workspace,
                             double* exact, hipStream_t stream);

// em2_gene_pairs.hip: ExpressionMatrix::findSimilarGenePairs0 (src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198) on a subset's
// CSR in device memory: the dense standardised gene vectors, r of every unordered pair of genes (float products and float sums
// in ascending cell order, no FMA), the survivors' stream, its sort and keepBest per gene.  d_pairs [geneCount][k] / d_used
// [geneCount] hold every gene's kept candidates in the arrangement std::nth_element leaves (unused slots zero): the caller runs
// the final std::sort (host::sortGenePairs).  method: the NormalizationMethod enum (0 none, 1 L1, 2 L2).  d_all: NULL or
// [geneCount][geneCount], every r off the diagonal.  Allocates its own scratch and synchronises the stream.
constexpr uint64_t kGenePairsBytesPerRecord = 24;         // key and value, twice (the sort alternates between two buffers)
struct GenePairsStatus {
    uint32_t inputError = 0;      // as runFsp0's; nothing was computed then
    bool overflow = false;        // more survivors than the stream's budget AND than the device has memory for: nothing was selected
    uint64_t records = 0;         // survivors, both directions counted
    uint64_t freeBytes = 0;       // with overflow: what the device had free when the exact size was refused
    int runs = 0;                 // of the pair kernel (2: the stream had to be sized exactly)
    uint32_t longestList = 0;     // the longest candidate list that needed a selection
};
void setGenePairsBudgetMegabytes(uint64_t megabytes);       // em2_set_gene_pairs_buffer_mb; 4096 until it is called
uint64_t genePairsBudgetRecords();
hipError_t runGenePairs(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, int method, uint32_t k,
                        double similarityThreshold, PairOut* d_pairs, uint32_t* d_used, float* d_all, GenePairsStatus* status,
                        hipStream_t stream);

// em2_gene_information.hip: ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) and the cells
// expressing every gene (src/ExpressionMatrixGeneSets.cpp:336-350) on a subset's CSR in device memory (toc from 0, entryCount
// entries).  d_normInverse: NULL (no normalisation) or the cells' norm1Inverse / norm2Inverse; launchCellNormInverses computes
// them (method 1 or 2) from the cells' WHOLE rows as addCell does (:241-263).  logN = log(double(cellCount)) and log2 = log(2.)
// come from the host's log.  d_informationContentDouble and d_expressingCellCount may be NULL.  *inputError != 0: nothing was
// computed (bits 0, 1: as runFsp0's; bit 2: toc does not cover exactly entryCount entries, ascending from 0).  Synchronises the stream.
constexpr uint32_t kGeneInformationChunk = 1024;          // entries of a gene one wave reduces (the reduction's shape)
size_t geneInformationWorkspaceBytes(uint64_t entryCount, uint32_t geneCount);
void setGeneInformationMaxBlocks(uint32_t blocks);      // em2_set_gene_information_max_blocks; 0 (the default): 65536
hipError_t launchCellNormInverses(const uint64_t* toc, const CountIn* data, uint32_t cellCount, uint32_t geneCount, int method,
                                  double* normInverse, hipStream_t stream);
hipError_t runGeneInformation(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                              const double* d_normInverse, double logN, double log2, float* d_informationContent,
                              double* d_informationContentDouble, uint32_t* d_expressingCellCount, void* workspace, size_t workspaceBytes,
                              uint32_t* inputError, hipStream_t stream);

// em2_rank_genes.hip: the integers of the rank-sum test of every gene for every group of cells against the rest (DESIGN.md
// 3.25) on a subset's CSR in device memory, as runGeneInformation takes it.  d_group[cellCount]: a group below groupCount or
// kNoGroup.  The outputs are [geneCount][groupCount] (d_groupSize [groupCount], d_tieSum [geneCount]).  *inputError != 0:
// nothing was written outside the workspace (bits 0-2: as runGeneInformation's; bit 3: a value is NaN; bit 4: a group id is
// neither below groupCount nor kNoGroup).  The caller has checked the limits (rankGenesUnsupported).  Synchronises the stream.
constexpr uint32_t kNoGroup = 0xffffffffu;
const char* rankGenesUnsupported(uint64_t cellCount, uint64_t geneCount, uint64_t entryCount, uint64_t groupCount);   // NULL: supported
const char* rankGenesErrorText(uint32_t inputError);
size_t rankGenesWorkspaceBytes(uint64_t entryCount, uint32_t geneCount, uint32_t groupCount);
void setRankGenesTestLimits(uint32_t maxBlocks, uint32_t chunkEntries, uint32_t ldsGroupLimit);     // em2_set_rank_genes_test_limits
hipError_t runRankGenes(const uint64_t* d_toc, const CountIn* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                        const double* d_normInverse, const uint32_t* d_group, uint32_t groupCount, uint32_t* d_groupSize,
                        uint32_t* d_nonZeroCount, uint64_t* d_rankSum2, uint64_t* d_tieSum, void* workspace, size_t workspaceBytes,
                        uint32_t* inputError, hipStream_t stream);

// em2_dense.hip: getDenseExpressionMatrix (src/PythonModule.cpp:112-138) for the rows [rowBegin, rowEnd) of a cell list (NULL: the
// CSR's own rows) into d_out[(row - rowBegin) * pitchElements + gene], floats or doubles; d_geneLocalIds NULL: the CSR is in
// local ids already.  *inputError != 0 (walkCell's word over the kept entries): nothing was written.  Synchronises the stream.
size_t denseExpressionWorkspaceBytes(uint32_t rowCount);
hipError_t runDenseExpression(const uint64_t* d_toc, const CountIn* d_data, const uint32_t* d_cellIds, const uint32_t* d_geneLocalIds,
                              uint32_t globalGeneCount, uint32_t geneCount, int method, uint32_t rowBegin, uint32_t rowEnd,
                              bool elementsAreDouble, void* d_out, size_t pitchElements, void* workspace, size_t workspaceBytes,
                              uint32_t* inputError, hipStream_t stream);

}  // namespace em2

#endif
