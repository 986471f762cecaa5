/* em2_lsh.h -- C ABI of the MI355X implementation of ExpressionMatrix2's LSH similar-pairs path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.  Each entry point names the
 * reference interface it replaces (file:line under the ExpressionMatrix2 source tree).  The reference is a C++
 * library with a pybind11 module; a maintainer binds these functions from ExpressionMatrixLsh.cpp /
 * PythonModule.cpp as shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns EM2_OK (0) or an EM2_ERROR_* code; em2_last_error() returns the message of the
 *     last failure on the calling thread.  Where the reference throws std::runtime_error with a fixed text
 *     ("Gene set X does not exist." ...) the message is that text and the code is EM2_ERROR_RUNTIME.
 *   - "dev" functions take DEVICE pointers valid on the current HIP device and a hipStream_t passed as void*;
 *     they enqueue work and return without synchronising.  They never allocate.
 *   - the other compute functions take HOST pointers, run on the current HIP device and return when the
 *     result is in the output buffers.  They fail with EM2_ERROR_NO_DEVICE when no GPU is present: there is
 *     no CPU fallback in this library.
 *   - cell ids are local to the cell set, gene ids local to the gene set (src/SimilarPairs.hpp:28-33).
 */
#ifndef EM2_LSH_H
#define EM2_LSH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EM2_OK 0
#define EM2_ERROR_INVALID_ARGUMENT 1
#define EM2_ERROR_NO_DEVICE 2
#define EM2_ERROR_HIP 3
#define EM2_ERROR_IO 4
#define EM2_ERROR_RUNTIME 5
#define EM2_ERROR_UNSUPPORTED 6

/* Layout of std::pair<CellId, float> (src/SimilarPairs.hpp:53-56): one stored neighbour of a cell. */
typedef struct em2_pair {
    uint32_t cell;
    float similarity;
} em2_pair;

/* Layout of std::pair<GeneId, float> (src/ExpressionMatrixSubset.hpp:36): one stored expression count. */
typedef struct em2_count {
    uint32_t gene;
    float count;
} em2_count;

int em2_abi_version(void);
const char* em2_last_error(void);

/* ------------------------------------------------------------------------------------------------------
 * Host-side pieces of the path (no GPU needed).
 * ------------------------------------------------------------------------------------------------------ */

/* Lsh::generateLshVectors (src/Lsh.cpp:68-113).  vectors is gene-major [geneCount][lshCount] like
 * Lsh::lshVectors (src/Lsh.hpp:104-113).  Generator: mt19937(seed) + the Box-Muller normal_distribution of
 * Boost <= 1.55, normalised per hyperplane.  Boost is not vendored by the reference and its
 * normal_distribution changed algorithm in 1.56, so a bit-for-bit match with a particular reference build is
 * not claimed: pass that build's own hyperplanes to em2_compute_signatures instead ("Oracle"). */
int em2_lsh_generate_vectors(uint32_t geneCount, uint32_t lshCount, uint32_t seed, double* vectors);

/* Lsh::computeSimilarityTable (src/Lsh.cpp:229-249): table[m] = cos(m*pi/lshCount), m = 0..lshCount. */
int em2_lsh_similarity_table(uint32_t lshCount, double* table);

/* MurmurHash64A as used by MemoryMapped::Vector::hash (src/MemoryMappedVector.hpp:715-723, seed 231). */
uint64_t em2_murmur_hash_64a(const void* key, int len, uint64_t seed);

/* ------------------------------------------------------------------------------------------------------
 * Device management.
 * ------------------------------------------------------------------------------------------------------ */
int em2_device_count(int* count);
int em2_set_device(int device);

/* ------------------------------------------------------------------------------------------------------
 * Host-buffer entry points: what a reference-side binding calls.
 * ------------------------------------------------------------------------------------------------------ */

/* ExpressionMatrixSubset::computeSums (src/ExpressionMatrixSubset.cpp:47-58) + Lsh::computeCellLshSignatures
 * (src/Lsh.cpp:118-224).  CSR: toc[cellCount+1] offsets into data, gene ids ascending within a cell and
 * < geneCount.  vectors as above.  signatures: cellCount * ((lshCount-1)/64+1) words, cell-major, bit i of a
 * cell in word i>>6 at bit position 63-(i&63) (src/BitSet.hpp:48-62). */
int em2_compute_signatures(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                           const double* vectors, uint32_t lshCount, uint64_t* signatures);

/* The pair loop, selection and storage order of ExpressionMatrix::findSimilarPairs4
 * (src/ExpressionMatrixLsh.cpp:200-285) + SimilarPairs::copy/sort (src/SimilarPairs.cpp:369-405).
 * pairs: cellCount*k slots, cell c at [c*k, c*k+usedCount[c]), sorted by similarity descending then cell id
 * ascending; unused slots are zero (as in a freshly created SimilarPairs-*-Pairs file). */
int em2_find_similar_pairs4(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                            double similarityThreshold, em2_pair* pairs, uint32_t* usedCount);

/* ExpressionMatrix::findSimilarPairs7 after its lookups (src/ExpressionMatrixLsh.cpp:563-690 with
 * findSimilarPairs7AssignCellsToBuckets :727-827): LSH buckets of several slice lengths (decreasing, each 1..64 bits;
 * buckets of slices with at least log2BucketCount bits are MurmurHash64A(value, seed 231) & (2^log2BucketCount - 1)),
 * per cell the first maxCheck distinct bucket-mates in (length, slice, id) order, of those the k with the fewest
 * mismatches among the ones with mismatchCount < Lsh::computeMismatchCountThresholdFromSimilarityThreshold
 * (src/Lsh.hpp:86-95), ascending (mismatch, id).  maxCheck 0 behaves as in the reference: no limit (:657 follows a push_back), except that
 * the walk ends at the first bucket that leaves the candidate list empty (:663).
 * Errors carry the reference's texts ("The slice lengths are not in decreasing order.", "Each slice length can be at
 * most 64 bits.").  Limits: k <= 4096, log2BucketCount <= 40, directly indexed slices <= 40 bits. */
int em2_find_similar_pairs7(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                            double similarityThreshold, const int32_t* sliceLengths, uint32_t sliceLengthCount,
                            uint32_t maxCheck, uint32_t log2BucketCount, em2_pair* pairs, uint32_t* usedCount);

/* ExpressionMatrix::findSimilarPairs6 after its lookups (src/ExpressionMatrixLsh.cpp:880-1145, src/charikar.hpp): the
 * Charikar permutation search.  permutationCount bit permutations are drawn from one std::mt19937 seeded with `seed`
 * (iota + std::shuffle over all lshCount bits, first permutedBitCount kept); the cells are sorted by their permuted
 * prefixes per permutation; per cell a priority queue of pointers into those sorted lists (ordered by common prefix
 * length, ties as libstdc++'s heap leaves them) yields up to searchCount candidates; those with
 * similarityTable[mismatch] > similarityThreshold are kept, sorted by (similarity desc, id asc), deduplicated and cut
 * to k.  Layout of pairs/usedCount as em2_find_similar_pairs4.
 * Errors: "Argument permutationStoreBitCount N exceeds number of signature bits L" (the reference's text);
 * permutedBitCount 0 is EM2_ERROR_INVALID_ARGUMENT (the reference sizes 2^58 words there).  Limits
 * (EM2_ERROR_UNSUPPORTED): permutationCount <= 64, permutedBitCount <= 65472, min(searchCount,
 * permutationCount*(cellCount-1)) <= 8192. */
int em2_find_similar_pairs6(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                            double similarityThreshold, uint32_t permutationCount, uint32_t searchCount,
                            uint32_t permutedBitCount, int32_t seed, em2_pair* pairs, uint32_t* usedCount);

/* ExpressionMatrix::findSimilarPairs0 after its lookups (src/ExpressionMatrixFindSimilarPairs.cpp:57-82): the exact
 * all-pairs search on the CSR of an expression matrix subset (toc[0..cellCount], data; local gene ids below geneCount,
 * strictly ascending within a cell).  Per pair ExpressionMatrixSubset::computeCellSimilarity
 * (src/ExpressionMatrixSubset.cpp:47-58,83-133: float products, double sums in ascending gene order, the correlation
 * coefficient with separate multiplications, IEEE square root and division); a pair with similarity > similarityThreshold
 * (as doubles) is offered to both cells through SimilarPairs::add (src/SimilarPairs.cpp:170-232), each cell seeing its
 * candidates in ascending id of the other cell; SimilarPairs::sort (:399-405) at the end.  pairs[cellCount][k] (unused
 * slots zero) and usedCount as em2_find_similar_pairs4; lowestSimilarityIndex / lowestSimilarity [cellCount] are the
 * CellInfo fields as add leaves them (the index names the slot before the sort; 0xffffffff / FLT_MAX for a cell
 * that stored nothing).  Counts that are zero, infinite or NaN take part exactly as in the reference's loop; a similarity
 * that is NaN passes no threshold.  Where the reference is undefined (a replacement while the index is 0xffffffff: k
 * stored similarities of +inf or FLT_MAX, or k = 0 with +inf) the candidate is dropped.
 * Errors: similarityThreshold > 1 is EM2_ERROR_RUNTIME (CZI_ASSERT, :26); min(k, cellCount-1) > 4096 is
 * EM2_ERROR_UNSUPPORTED. */
int em2_find_similar_pairs0(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, uint32_t k,
                            double similarityThreshold, em2_pair* pairs, uint32_t* usedCount, uint32_t* lowestSimilarityIndex,
                            float* lowestSimilarity);

/* ExpressionMatrix::findSimilarGenePairs0 after its lookups (src/ExpressionMatrixFindSimilarGenePairs.cpp:77-188, with
 * ExpressionMatrixSubset::getDenseRepresentation, src/ExpressionMatrixSubset.cpp:142-174, and keepBest, src/heap.hpp:116-126):
 * the Pearson correlation of every pair of genes over the cells of a subset's CSR (as em2_find_similar_pairs0: local gene ids
 * below geneCount, strictly ascending within a cell).  Dense float vector per gene; cells scaled by float(1/sum1) (L1) or
 * float(1/sqrt(sum2)) (L2) where that sum is not zero, every entry of the cell, zeros included; per gene, over the cells in
 * ascending order: double sum, average = float(sum/cellCount), x -= average, double sum of the float squares, x *=
 * float(1/sqrt(sum2)); r = acc over the cells ascending of acc = acc + (x0*x1), float product and float sum, no FMA, subnormals
 * kept.  A pair with double(r) > similarityThreshold is a candidate of both genes (ascending partner id); a list longer than
 * k goes through libstdc++'s std::nth_element (restated, csrc/em2_select.h) and is cut to k; every list is sorted by
 * std::sort on the similarity alone (no tie-break on the id: ties are stored as those two algorithms leave them).  A gene
 * without variance gives NaN or inf by IEEE rules; NaN passes no threshold.
 * normalizationMethod: NormalizationMethod (src/NormalizationMethod.hpp:11-16) 0 none, 1 L1, 2 L2.
 * pairs[geneCount][k] (em2_pair.cell holds the partner's local gene id; unused slots zero), usedCount[geneCount].
 * allSimilarities: NULL, or [geneCount][geneCount] floats that receive every r (the diagonal 0): an aid for tests, refused
 * (EM2_ERROR_UNSUPPORTED) above 8192 genes.
 * The candidates pass through a device buffer of at most the megabytes em2_set_gene_pairs_buffer_mb set (default 4096; 24
 * bytes per candidate and direction), or of the worst case geneCount*(geneCount-1) if that is smaller; if there are more,
 * the pairs are evaluated once more into a buffer of the exact size, and if the device has no room for that the call fails
 * with EM2_ERROR_UNSUPPORTED, naming the count and the setter.  It never truncates.
 * em2_set_gene_pairs_buffer_mb is process-wide and takes effect for the calls that start after it; the Python binding calls
 * it with the environment variable EM2_GENE_PAIRS_BUFFER_MB before every findSimilarGenePairs0. */
void em2_set_gene_pairs_buffer_mb(uint64_t megabytes);
int em2_find_similar_gene_pairs0(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                 int normalizationMethod, uint32_t k, double similarityThreshold, em2_pair* pairs,
                                 uint32_t* usedCount, float* allSimilarities);

/* ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-2018) for every gene of a subset's CSR (as
 * em2_find_similar_pairs0: local gene ids below geneCount, strictly ascending within a cell; else EM2_ERROR_INVALID_ARGUMENT),
 * and the number of cells with a stored entry for the gene, stored zeros included (the counter of createWellExpressedGeneSet,
 * src/ExpressionMatrixGeneSets.cpp:336-350).  It replaces the reference's binary search per (gene, cell)
 * (getCellExpressionCount, :1035-1046) with one stable sort of the stored entries by gene and a segmented reduction.
 * normInverse: NULL (NormalizationMethod none) or [cellCount], the cells' Cell::norm1Inverse (L1) or norm2Inverse (L2): those
 * of the WHOLE cell over all genes (:1976), see em2_cell_norm_inverses.  c = count * float(normInverse) is a float product
 * (:1981-1992).  Per gene: sum = the double sum of c over its stored entries, whatever their sign; I = log(double(cellCount))
 * + the sum over c > 0 of p * log(p), p = double(c) * (1. / sum); I /= log(2.); informationContent = float(I) (:1997-2017).
 * IEEE rules decide the odd cases (an inf count gives NaN); where float(normInverse) of a cell is inf or NaN the reference's
 * product with the 0 of a gene the cell does not store is NaN, so every gene with a positive entry is NaN then.
 * Pinned bit for bit: expressingCellCount, and informationContent of a gene without a positive entry (log(double(cellCount))
 * and log(2.) are the host's, the gene gets float(logN / log2)); informationContent == float(informationContentDouble).  The
 * last bits of the double of an expressed gene are not pinned (the reference's depend on its libm's log and on a sequential
 * sum): they are held to an error bound, and they are a function of the input alone -- the same for every
 * call, for the host and the device entry, whatever the grid.
 * informationContentDouble and expressingCellCount may be NULL. */
int em2_gene_information_content(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                 const double* normInverse, float* informationContent, double* informationContentDouble,
                                 uint32_t* expressingCellCount);

/* The most blocks (of four waves) the wave-per-cell and wave-per-chunk kernels of the call are launched with; 0 restores the
 * default.  Process-wide and meant for this project's tests alone (the result does not depend on it, which is what they show
 * with it): unsupported elsewhere, and a call that runs while another thread changes it may size its launches by either value. */
void em2_set_gene_information_max_blocks(uint32_t blocks);

/* The same on device pointers and a stream: d_toc[cellCount + 1] non-decreasing from 0 to entryCount (else
 * EM2_ERROR_INVALID_ARGUMENT, and nothing is written outside the workspace), d_data[entryCount].  d_workspace: at
 * least em2_dev_gene_information_content_workspace bytes.  Synchronises the stream. */
size_t em2_dev_gene_information_content_workspace(uint32_t cellCount, uint32_t geneCount, uint64_t entryCount);
int em2_dev_gene_information_content(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                                     uint64_t entryCount, const double* d_normInverse, float* d_informationContent,
                                     double* d_informationContentDouble, uint32_t* d_expressingCellCount, void* d_workspace,
                                     size_t workspaceBytes, void* stream);

/* Rank-sum (Mann-Whitney / Wilcoxon) marker genes: for every gene of a subset's CSR and every group of cells, the test of the
 * group against the rest of the cells.  The reference has no such test (its compareClusters,
 * src/ExpressionMatrixHttpServerClusterGraphs.cpp:595-900, is a scatter plot of two averages).
 * Inputs: the CSR as em2_gene_information_content takes it (toc from 0, strictly ascending local gene ids below geneCount);
 * normInverse NULL or [cellCount]; group[cellCount], each a group below groupCount or EM2_NO_GROUP -- such a cell belongs to no
 * group but is part of every "rest"; groupCount >= 1.
 * Values: the value of cell c for gene g is count * float(normInverse[c]), one float product (the count itself where
 * normInverse is NULL), and +0 where the cell stores nothing for g, whatever the cell's factor.  -0 counts as +0.  +-inf are
 * ordinary values.  A NaN value fails the call with EM2_ERROR_INVALID_ARGUMENT ("a value is not a number").
 * Ranks of gene g, over all N = cellCount values: with m its stored entries sorted ascending at the positions 0 .. m-1,
 * z = N - m, neg = the stored values < 0, nz = the stored values != 0 and t0 = N - nz (every zero, stored or not, is one tie
 * group), TWICE the mid-rank of a value is
 *     a + b + 1            for a run of equal values < 0 at the positions [a, b),
 *     a + b + 1 + 2 z      for a run of equal values > 0 at the positions [a, b),
 *     2 neg + t0 + 1       for every zero.
 * Outputs, integers all, so that no sum has an order and every call gives the same bits:
 *     groupSize[groupCount]                       the cells of the group;
 *     nonZeroCount[geneCount][groupCount]         the cells of the group with a value != 0 for the gene;
 *     rankSum2[geneCount][groupCount]  (64 bits)  the sum over the cells of the group of twice the mid-rank;
 *     tieSum[geneCount]                (64 bits)  the sum of t^3 - t over all tie groups, the zeros' included.
 * zScore and auc ([geneCount][groupCount], each may be NULL) are host arithmetic on those integers, in the order that
 * csrc/em2_rank_genes_host.h states: with n the group's size and m = N - n, u2 = rankSum2 - n (n + 1) (twice U),
 * var = n m (N^3 - N - tieSum) / (12 N (N - 1)), z = 0.5 (u2 - n m) / sqrt(var) (0 where var is not positive; no continuity
 * correction), auc = u2 / (2 n m) (0.5 where n m = 0).  The two-sided p-value is erfc(|z| / sqrt(2)).
 * EM2_ERROR_UNSUPPORTED, before any launch: cellCount > 2^21 (t^3 would leave 64 bits), 2^32 entries or more,
 * geneCount * groupCount > 2^28. */
#define EM2_NO_GROUP 0xffffffffu
int em2_rank_genes(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, const double* normInverse,
                   const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2,
                   uint64_t* tieSum, double* zScore, double* auc);

/* The integers of em2_rank_genes on device pointers and a stream (d_toc and d_data as em2_dev_gene_information_content takes
 * them).  On an input error (EM2_ERROR_INVALID_ARGUMENT: the toc, a gene id, a NaN value, a group id that is neither below
 * groupCount nor EM2_NO_GROUP) nothing is written outside the workspace.  d_workspace: at least
 * em2_dev_rank_genes_workspace bytes (0: the shape is not supported).  Synchronises the stream. */
size_t em2_dev_rank_genes_workspace(uint32_t cellCount, uint32_t geneCount, uint64_t entryCount, uint32_t groupCount);
int em2_dev_rank_genes(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount, uint64_t entryCount,
                       const double* d_normInverse, const uint32_t* d_group, uint32_t groupCount, uint32_t* d_groupSize,
                       uint32_t* d_nonZeroCount, uint64_t* d_rankSum2, uint64_t* d_tieSum, void* d_workspace, size_t workspaceBytes,
                       void* stream);

/* The most blocks any kernel of the call is launched with, the entries of a gene one workgroup of the accumulate pass takes
 * (a chunk), and the largest groupCount whose counters that pass keeps in LDS (above it the adds go straight to global memory;
 * at most 4096).  0 restores each default (16384 blocks, 2048 entries, 4096 groups).  The workspace size depends on the chunk:
 * ask for it after the call.  Process-wide and meant for this project's tests alone (the result does not depend on any of
 * them, which is what they show with it): unsupported elsewhere, and a call that runs while another thread changes them may
 * size its launches by either value. */
void em2_set_rank_genes_test_limits(uint32_t maxBlocks, uint32_t chunkEntries, uint32_t ldsGroupLimit);

/* Cell::norm1Inverse and norm2Inverse as ExpressionMatrix::addCell defines them (src/ExpressionMatrix.cpp:241-263) for the
 * cells of a CSR: sum1 += value, sum2 += value * value (a float product), both sums double, in stored order;
 * 1. / sum1 and 1. / sqrt(sum2).  (The reference sums in the order of ingest, before it sorts the row by gene id.)  Host
 * code; the gene ids are checked as above. */
int em2_cell_norm_inverses(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount, double* norm1Inverse,
                           double* norm2Inverse);

/* ExpressionMatrix::getDenseExpressionMatrix (src/PythonModule.cpp:78-154, the arithmetic :112-138; bound at :479-496) on the
 * GPU: out[cell][gene], row-major, zero where the cell stores nothing for the gene.  (NOT getDenseRepresentation of
 * findSimilarGenePairs0, which is gene-major, float, and guards a zero sum.)
 *   factor of a cell (:117-130)   none: 1.f    L1: float(1. / sum1)    L2: float(1. / sqrt(sum2)),
 *   sum1, sum2 = ExpressionMatrixSubset::computeSums (src/ExpressionMatrixSubset.cpp:47-58) over the cell's entries WITHIN THE
 *   GENE SET in stored order: doubles; count * count is a float product.  Every stored entry becomes double(factor * count), a
 *   float product, then widened (:135-136).  There is no guard against a zero sum, as in the reference: a cell whose kept
 *   entries are all stored zeros gives inf * 0 = NaN at those entries (0 elsewhere), a cell without a kept entry is a row of
 *   zeros, counts that cancel give +-inf.  The sign and payload of such a NaN are the hardware's.
 * elementType: EM2_DENSE_FLOAT64 is the reference's array.  EM2_DENSE_FLOAT32 holds the same values -- every element is a float
 * before the reference widens it -- in half the bytes.
 *
 * em2_dev_dense_expression: everything in device memory.  The rows [rowBegin, rowEnd) of the result, rowEnd <= cellCount, go to
 * d_out[(row - rowBegin) * pitchElements + gene]; pitchElements >= geneCount, and what lies behind geneCount in a row is not
 * touched.  d_cellIds NULL: row r is cell r of the CSR; else row r is cell d_cellIds[r], cellCount ids (as em2_dev_subset_*;
 * like there, the ids are the caller's to vouch for: this entry is not told how many cells the CSR has).  d_geneLocalIds
 * NULL: the CSR is in local ids already; else it is GeneSet-<name>-LocalIds of globalGeneCount words (0xffffffff: not in the
 * set) and the CSR holds global ids: the gene mapping is fused, no restricted CSR is built.  geneCount is the gene set's size.
 * A kept gene id not below geneCount, or kept ids not strictly ascending within a cell: EM2_ERROR_INVALID_ARGUMENT and nothing
 * is written.  d_out is aligned to its element; the workspace is em2_dev_dense_expression_workspace(rowEnd - rowBegin) bytes.
 * Synchronises the stream.
 *
 * em2_dense_expression: the same on host buffers, the whole matrix (cellCount rows into out[row * pitchElements + gene]),
 * through a device buffer of at most 1 GiB.  toc / data have csrCellCount cells; cellIds NULL: cellCount == csrCellCount.
 * A cell id not below csrCellCount: EM2_ERROR_INVALID_ARGUMENT (the reference reads out of bounds). */
#define EM2_DENSE_FLOAT64 0
#define EM2_DENSE_FLOAT32 1
size_t em2_dev_dense_expression_workspace(uint32_t rowCount);
int em2_dev_dense_expression(const uint64_t* d_toc, const em2_count* d_data, const uint32_t* d_cellIds, uint32_t cellCount,
                             const uint32_t* d_geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                             uint32_t rowBegin, uint32_t rowEnd, int elementType, void* d_out, uint64_t pitchElements,
                             void* d_workspace, size_t workspaceBytes, void* stream);
int em2_dense_expression(const uint64_t* toc, const em2_count* data, uint32_t csrCellCount, const uint32_t* cellIds, uint32_t cellCount,
                         const uint32_t* geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                         int elementType, void* out, uint64_t pitchElements);

/* ------------------------------------------------------------------------------------------------------
 * Colouring and drawing a laid-out graph (ExpressionMatrix::exploreCellGraph, src/ExpressionMatrixHttpServerGraphs.cpp:350-1150,
 * and CellGraph::writeSvg, src/CellGraph.cpp:301-439; csrc/em2_cell_values.hip, em2_draw.hip, em2_draw_host.cpp).
 * ------------------------------------------------------------------------------------------------------
 * Values per cell.  Both read a CSR with d_geneLocalIds as em2_dev_dense_expression does (NULL: local ids already), cellCount
 * cells, and a list of `count` cells (d_cellIds NULL: the cells 0 .. count - 1).  A listed cell id not below cellCount, a kept
 * gene id not below geneCount and kept ids that do not ascend within a cell are EM2_ERROR_INVALID_ARGUMENT; what out then holds
 * is unspecified.  Both synchronise the stream.
 *
 * em2_dev_cell_similarities_to_cell: out[i] = ExpressionMatrix::computeCellSimilarity(geneSet, cellId0, cellIds[i])
 * (src/ExpressionMatrix.cpp:1468-1537), the reference's double: sum01 from the float products of the genes both cells keep, in
 * ascending gene order, widened to double; sum0, sum00, sum1, sum11 over each cell's kept entries in stored order (count * count
 * a float product); n = geneCount; (n sum01 - sum0 sum1) / sqrt((n sum00 - sum0^2)(n sum11 - sum1^2)) with no guard, so a cell
 * without a kept entry gives 0/0 = NaN.  Where the NaN sits is the contract; its sign and payload are the hardware's.  Presence,
 * not the value, decides what both cells have: a stored zero, inf or NaN takes part as in the reference's merge loop.  cellId0
 * need not be listed and is computed like any other cell where it is.  Cell 0 as a dense vector lives in LDS, or in the workspace
 * for gene sets that do not fit (em2_cell_similarities_row_in_lds(geneCount) says which: 1 for LDS).  The workspace is
 * em2_dev_cell_similarities_to_cell_workspace(geneCount, count) bytes.
 *
 * em2_dev_gene_expression_of_cells: out[i] = the value ExpressionMatrix::computeExpressionVector (:1253-1296) gives gene
 * globalGeneId in cell cellIds[i], as the page stores it (src/ExpressionMatrixHttpServerGraphs.cpp:817-833): factor * count, a
 * float product, with the factor of em2_dev_dense_expression over the kept entries; 0 where the cell stores nothing for the
 * gene.  It is column localGene of em2_dev_dense_expression's EM2_DENSE_FLOAT32 matrix, NaN for a stored zero in a zero-sum cell
 * included.  (globalGeneId is a local id where d_geneLocalIds is NULL.)  A gene outside the gene set is the reference's
 * CZI_ASSERT at :821: EM2_ERROR_RUNTIME.  The workspace is em2_dev_gene_expression_of_cells_workspace() bytes.
 *
 * The forms without _dev take host buffers; the em2_matrix_ forms a gene set of the directory and global cell ids, and send only
 * the rows they need to the device.  "Gene set X does not exist." as everywhere. */
size_t em2_dev_cell_similarities_to_cell_workspace(uint32_t geneCount, uint32_t count);
int em2_cell_similarities_row_in_lds(uint32_t geneCount);
int em2_dev_cell_similarities_to_cell(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                                      uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* d_cellIds,
                                      uint32_t count, double* d_out, void* d_workspace, size_t workspaceBytes, void* stream);
int em2_cell_similarities_to_cell(const uint64_t* toc, const em2_count* data, uint32_t cellCount, const uint32_t* geneLocalIds,
                                  uint32_t globalGeneCount, uint32_t geneCount, uint32_t cellId0, const uint32_t* cellIds, uint32_t count,
                                  double* out);
size_t em2_dev_gene_expression_of_cells_workspace(void);
int em2_dev_gene_expression_of_cells(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, const uint32_t* d_geneLocalIds,
                                     uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int normalizationMethod,
                                     const uint32_t* d_cellIds, uint32_t count, float* d_out, void* d_workspace, size_t workspaceBytes,
                                     void* stream);
int em2_gene_expression_of_cells(const uint64_t* toc, const em2_count* data, uint32_t cellCount, const uint32_t* geneLocalIds,
                                 uint32_t globalGeneCount, uint32_t geneCount, uint32_t globalGeneId, int normalizationMethod,
                                 const uint32_t* cellIds, uint32_t count, float* out);

/* Colours from numbers (src/ExpressionMatrixHttpServerGraphs.cpp:1003-1040 with spectralColor and color of src/color.cpp:13-79).
 * minValue / maxValue are found over the values: numeric_limits<double>::max() is skipped as "no value", and a NaN never
 * replaces a bound (std::min / std::max compare with <).  minColorValue / maxColorValue are the arguments where haveMin /
 * haveMax say so, else minValue / maxValue.  If minValue == maxValue, or there is no value at all, every rgb is EM2_COLOR_BLACK
 * (the page's "black").  Otherwise x = (1. / (maxColorValue - minColorValue)) * (value - minColorValue), red (x <= 0) through
 * yellow (0.5) to green (x >= 1), clipped, int(c * 255): doubles, one rounding per operation.  A NaN value falls through every
 * comparison and is 0x00ff00, as in the reference.  A value equal to max() is EM2_COLOR_NONE (the page leaves such a vertex the
 * colour it had).  rgb[i] is 0x00rrggbb, or one of the two flags with zero colour bits; the string of a colour is
 * "#%02x%02x%02x" of the same integers.  range[4] = minValue, maxValue, minColorValue, maxColorValue (max() and lowest() where
 * there is no value; the sign of a bound that is zero is unspecified, nothing depends on it).  The workspace is
 * em2_dev_spectral_colors_workspace() bytes.  em2_dev_spectral_colors does not synchronise. */
#define EM2_COLOR_NONE 0x80000000u
#define EM2_COLOR_BLACK 0x40000000u
size_t em2_dev_spectral_colors_workspace(void);
int em2_dev_spectral_colors(const double* d_values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                            uint32_t* d_rgb, double* d_range, void* d_workspace, size_t workspaceBytes, void* stream);
int em2_spectral_colors(const double* values, uint64_t count, double minColorValue, double maxColorValue, int haveMin, int haveMax,
                        uint32_t* rgb, double* range);

/* The number a meta data value stands for when the page colours by it (:949-964): the whole string is given to strtod, with no
 * leading white space allowed; anything else gives numeric_limits<double>::max(), "no value".  The reference uses
 * boost::lexical_cast<double>: parity with Boost on exotic spellings ("inf", hexadecimal, a trailing "f") is unpinned. */
int em2_meta_data_number(const char* value, uint64_t bytes, double* number);

/* The raster of a laid-out graph: the painter's result of CellGraph::writeSvg without anti-aliasing, this project's own
 * definition.  Any graph as plain arrays, like em2_graph_layout.  No result depends on an order between threads, and everything
 * after one conversion of the coordinates is integer arithmetic.
 *   S = sizePixels, 1 <= S <= 8192.  xMin = xViewBoxCenter - viewBoxHalfSize, likewise yMin; the y axis points down as SVG's does.
 *   s256 = double(S) * 256. / (2. * viewBoxHalfSize).  Per vertex ux = floor((x - xMin) * s256) clamped to +-2^30, likewise uy; the
 *   vertex's pixel is (ux >> 8, uy >> 8), an arithmetic shift.
 *   Vertices: R = llround(vertexRadius * s256).  Pixel (i, j) is covered by a vertex iff (256 i + 128 - ux)^2 + (256 j + 128 - uy)^2
 *   <= R^2 in 64-bit integers, or it is the vertex's own pixel (no vertex inside the image vanishes).  vertexTop[j * S + i] is the
 *   largest index + 1 among the covering vertices, 0 if none: a later vertex is on top, as in the SVG, and the caller passes the
 *   vertices in painter order.
 *   Edges, unless hideEdges: a one-pixel line from the pixel of v0 to the pixel of v1, as stored.  The major axis is x if
 *   |dx| >= |dy|, else y; dM and dm are the absolute extents; step k = 0 .. dM lies at major0 + sign k,
 *   minor0 + sign floor((2 k dm + dM) / (2 dM)) (dM = 0: one pixel).  Steps outside the image are never touched.  edgeHits[p]
 *   is the number of (edge, step) pairs that land on p.  The reference's default edge thickness is 0.05 pixel, a hairline: the
 *   raster ignores thickness.
 * EM2_ERROR_INVALID_ARGUMENT, and nothing is written: a position that is not finite, viewBoxHalfSize <= 0 or not finite, a radius
 * above 256 pixels or negative, S out of range, an edge end not below vertexCount, edgeCount >= 2^32, vertexCount = 2^32 - 1.
 * Work split: a lane per vertex for radii up to 4 pixels, a wave above; a lane per edge, and a wave for an edge with more than
 * em2_graph_draw_long_edge_steps() steps inside the image.  The workspace is em2_dev_graph_draw_workspace(vertexCount, edgeCount)
 * bytes.  em2_dev_graph_draw synchronises the stream.
 *
 * em2_dev_graph_compose: rgba[p] = white; where edgeHits > 0 the grey 255 - min(255, edgeShade * hits), edgeShade in [1, 255] (255
 * is the SVG's black, smaller values give a density picture); where vertexTop > 0 the low 24 bits of vertexRgb[vertexTop - 1]
 * (EM2_COLOR_NONE and EM2_COLOR_BLACK are black; vertexRgb NULL: every vertex black).  Bytes r, g, b, a = 255.  Does not
 * synchronise.  The host form checks vertexTop against vertexCount. */
uint32_t em2_graph_draw_long_edge_steps(void);
size_t em2_dev_graph_draw_workspace(uint32_t vertexCount, uint64_t edgeCount);
int em2_dev_graph_draw(uint32_t vertexCount, const double* d_x, const double* d_y, uint64_t edgeCount, const uint32_t* d_v0,
                       const uint32_t* d_v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                       double viewBoxHalfSize, double vertexRadius, uint32_t* d_vertexTop, uint32_t* d_edgeHits, void* d_workspace,
                       size_t workspaceBytes, void* stream);
int em2_graph_draw(uint32_t vertexCount, const double* x, const double* y, uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1,
                   int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter, double viewBoxHalfSize,
                   double vertexRadius, uint32_t* vertexTop, uint32_t* edgeHits);
int em2_dev_graph_compose(uint32_t sizePixels, const uint32_t* d_vertexTop, const uint32_t* d_edgeHits, const uint32_t* d_vertexRgb,
                          uint32_t edgeShade, uint8_t* d_rgba, void* stream);
int em2_graph_compose(uint32_t sizePixels, const uint32_t* vertexTop, const uint32_t* edgeHits, const uint32_t* vertexRgb,
                      uint32_t vertexCount, uint32_t edgeShade, uint8_t* rgba);

/* CellGraph::writeSvg (src/CellGraph.cpp:301-439) into a file, byte for byte for the same doubles and strings: the edges group
 * first unless hideEdges (every edge "black": no edge has a colour of its own here), the xlink:href with geneSetName, ostream's
 * default formatting (precision 6).  groupColorCount == 0 is the reference's empty groupColors map: one circle per vertex in
 * vertex order, fill='<colour>' where vertexColors (vertexCount strings, each followed by a 0 byte; NULL: none) has a string
 * that is not empty.  Otherwise the vertices group by group in ascending group order (vertexGroups[v]), every group in vertex
 * order, with the colour the map (groupColorGroups[g] -> g-th string of groupColors) gives the group and "black" for a group
 * without one.  Host only. */
int em2_graph_write_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint32_t* cellIds,
                        uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels,
                        double xViewBoxCenter, double yViewBoxCenter, double viewBoxHalfSize, double vertexRadius, double edgeThickness,
                        const char* vertexColors, uint64_t vertexColorsBytes, const uint32_t* vertexGroups, uint32_t groupColorCount,
                        const int32_t* groupColorGroups, const char* groupColors, uint64_t groupColorsBytes, const char* geneSetName);

/* ------------------------------------------------------------------------------------------------------
 * Colouring and drawing the signature graph: pie vertices (ExpressionMatrix::colorBlack, colorRandom and
 * colorByMetaDataInterpretedAsCategory, src/ExpressionMatrixSignatureGraph.cpp:163-278, and SignatureGraph::writeSvg,
 * src/SignatureGraph.cpp:183-321; csrc/em2_pie.hip, em2_pie_host.cpp).
 * ------------------------------------------------------------------------------------------------------
 * The colour census.  A vertex owns the cells cells[cellOffsets[v] .. cellOffsets[v + 1]) (ids into a cell set of cellSetSize
 * cells, as em2_signature_graph_get gives them; cellCount is the length of cells[], below 2^32), a cell has the value id
 * idOfCell[cell] < valueCount, a value the colour index colorOfValue[id] in 0 .. 12 (12 is "black": every value from the
 * thirteenth rank on).  Per vertex, over its cells in stored order (:230-262): the cells of each colour index, the colours that
 * occur in order of first occurrence, sorted by count descending with first occurrence deciding among equal counts (std::sort
 * of at most 13 elements is libstdc++'s insertion sort, which is stable), sum = the sum of the counts, factor = 1. / sum,
 * fraction = count * factor: doubles with one rounding each, the reference's bits.  The result is a CSR over the vertices:
 * sliceOffsets [vertexCount + 1], and per slice sliceColor (0 .. 12), sliceCells and sliceFraction.  A vertex without cells has
 * no slice.  Every id is tested before an address is formed with it: a cell not below cellSetSize, a value id not below
 * valueCount, a colour index above 12, or offsets that do not ascend within cellCount are EM2_ERROR_INVALID_ARGUMENT, and no
 * object is made.  Work split: a lane per vertex of at most em2_pie_census_wave_cells() cells, a wave per vertex above; a vertex
 * of 10^6 cells is worked by that one wave, a known limit.  No result depends on an order between threads.
 * The result is an object: em2_pie_census_sizes (any may be NULL; waveVertexCount: the vertices a wave worked), then
 * em2_pie_census_get into arrays of those sizes (any may be NULL).  em2_dev_pie_census takes device pointers.
 *
 * em2_matrix_pie_census (declared with the em2_matrix_ entries below) is colorByMetaDataInterpretedAsCategory for a graph whose vertices hold ids into globalCellIds
 * [cellSetSize]: the host walks the meta data lists of those cells once and writes one compact value id per cell, as
 * em2_matrix_compute_meta_data_rand_index does (a cell without the field and a stored "" share an id; a field name the store
 * does not know gives every cell "", as getCellMetaData(CellId, StringId) does for the invalid name id: one value, no error);
 * the device counts the cells of each value over the cells of the vertices (em2_contingency_create with one column); the host
 * puts the values that occur, in std::map order (string ascending), through std::sort with OrderPairsBySecondGreater
 * (em2_order_by_count) and gives rank r the colour index min(r, 12); then the census above.  The object then also holds the
 * value table in that sorted order: em2_pie_census_values_sizes, then em2_pie_census_values_get (values: the strings, each
 * followed by a 0 byte). */
typedef struct em2_pie_census em2_pie_census;
uint32_t em2_pie_census_wave_cells(void);
int em2_pie_census_create(uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                          const uint32_t* idOfCell, uint32_t cellSetSize, const uint8_t* colorOfValue, uint32_t valueCount,
                          em2_pie_census** census);
int em2_dev_pie_census(uint32_t vertexCount, const uint64_t* d_cellOffsets, const uint32_t* d_cells, uint64_t cellCount,
                       const uint32_t* d_idOfCell, uint32_t cellSetSize, const uint8_t* d_colorOfValue, uint32_t valueCount,
                       em2_pie_census** census);
int em2_pie_census_sizes(const em2_pie_census* census, uint32_t* vertexCount, uint64_t* sliceCount, uint32_t* waveVertexCount);
int em2_pie_census_get(const em2_pie_census* census, uint64_t* sliceOffsets, uint8_t* sliceColor, uint32_t* sliceCells,
                       double* sliceFraction);
int em2_pie_census_values_sizes(const em2_pie_census* census, uint64_t* valueCount, uint64_t* valueBytes);
int em2_pie_census_values_get(const em2_pie_census* census, char* values, uint64_t* valueCells);
void em2_pie_census_free(em2_pie_census* census);

/* order[] = the indices 0 .. count - 1 as std::sort leaves the pairs (index, counts[index]) under the reference's
 * OrderPairsBySecondGreater (src/orderPairs.hpp:56-62), which looks at the count alone: std::sort is not stable above 16
 * elements, and the order of equal counts is libstdc++'s; it depends on the comparator's results only, so this calls std::sort
 * and restates nothing.  Both the value table of em2_matrix_pie_census and the painter order of the signature graph's vertices
 * (sortedVertices, src/SignatureGraph.cpp:234-239) are this.  Host only. */
int em2_order_by_count(const uint64_t* counts, uint64_t count, uint32_t* order);

/* colorRandom (:176-194): per vertex, in vertex order, three draws of std::uniform_real_distribution<double>(0, 1.) from one
 * std::mt19937(231), through color() of src/color.cpp:13-39 (clipped to [0, 1], int(c * 255)): rgb[v] = 0x00rrggbb, whose string
 * is "#%02x%02x%02x".  <random> itself is called.  Host only. */
int em2_signature_graph_random_colors(uint32_t vertexCount, uint32_t* rgb);

/* The raster of a laid-out graph whose vertices are pie charts, this project's own definition.  Any graph as plain arrays.  The
 * view, ux / uy, the own-pixel rule, the edge layer and edgeHits, the long-edge split and their checks are em2_graph_draw's,
 * word for word (the same code runs).  After one conversion per vertex everything is integer arithmetic, and no result
 * depends on an order between threads.
 *   Vertices: the caller passes them in painter order (a later index is on top); vertex v has its own radius[v], in the
 *   layout's units.  R_v = llround(radius[v] * s256).  Pixel (i, j) is covered by v iff (256 i + 128 - ux)^2 + (256 j + 128 -
 *   uy)^2 <= R_v^2, or it is v's own pixel; vertexTop[j * S + i] is the largest index + 1 among the covering vertices, 0 if
 *   none.  The bounding box is clipped to the image, so a vertex costs at most S^2 tests.
 *   Slices: vertex v has the slices sliceOffsets[v] .. sliceOffsets[v + 1] - 1, at least one (sliceOffsets [vertexCount + 1]
 *   begins at 0, ascends strictly and ends at sliceCount < 2^32 - 1).  Slice k starts at the direction (boundaryX[k],
 *   boundaryY[k]), int32, and ends where the vertex's next slice starts, the last one where the first starts; largeArc[k] != 0
 *   says that it spans more than half a turn.  The y axis points down in the raster as in the SVG, so the SVG's sweep flag 1 is
 *   the direction of increasing angle in these coordinates.  With cross(p, q) = p.x q.y - p.y q.x in 64-bit integers, the
 *   sector from a to b holds d iff cross(a, d) >= 0 && cross(d, b) > 0 when largeArc is 0, and iff
 *   !(cross(b, d) >= 0 && cross(d, a) > 0) when it is not.  Once vertexTop is final, pixel p with the top vertex v and
 *   d = (256 i + 128 - ux, 256 j + 128 - uy) belongs to v's first slice if v has one slice or d = (0, 0); otherwise to the first
 *   of v's slices but the last whose sector holds d, else to the last.  sliceTop[p] = that slice's index + 1, 0 where vertexTop[p]
 *   is 0.  em2_dev_graph_compose then takes sliceTop and a colour per slice, unchanged.
 * EM2_ERROR_INVALID_ARGUMENT, and nothing is written: what em2_graph_draw refuses, a radius that is negative, not finite or above
 * 8192 pixels, slice offsets that are not as above.
 * Work split by radius class: a lane per vertex up to 4 pixels, a wave per vertex up to em2_graph_draw_pies_wave_radius() pixels,
 * a workgroup per vertex above; the vertices are compacted into the three classes on the device, in any input order.  The
 * workspace is em2_dev_graph_draw_pies_workspace(vertexCount, edgeCount) bytes.  em2_dev_graph_draw_pies synchronises the stream. */
double em2_graph_draw_pies_wave_radius(void);
size_t em2_dev_graph_draw_pies_workspace(uint32_t vertexCount, uint64_t edgeCount);
int em2_dev_graph_draw_pies(uint32_t vertexCount, const double* d_x, const double* d_y, const double* d_radius, uint64_t edgeCount,
                            const uint32_t* d_v0, const uint32_t* d_v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter,
                            double yViewBoxCenter, double viewBoxHalfSize, const uint64_t* d_sliceOffsets, uint64_t sliceCount,
                            const int32_t* d_boundaryX, const int32_t* d_boundaryY, const uint8_t* d_largeArc, uint32_t* d_vertexTop,
                            uint32_t* d_sliceTop, uint32_t* d_edgeHits, void* d_workspace, size_t workspaceBytes, void* stream);
int em2_graph_draw_pies(uint32_t vertexCount, const double* x, const double* y, const double* radius, uint64_t edgeCount, const uint32_t* v0,
                        const uint32_t* v1, int hideEdges, uint32_t sizePixels, double xViewBoxCenter, double yViewBoxCenter,
                        double viewBoxHalfSize, const uint64_t* sliceOffsets, uint64_t sliceCount, const int32_t* boundaryX,
                        const int32_t* boundaryY, const uint8_t* largeArc, uint32_t* vertexTop, uint32_t* sliceTop, uint32_t* edgeHits);

/* The boundary vectors of em2_graph_draw_pies from the fractions of a census, in the SVG's doubles (src/SignatureGraph.cpp:297-
 * 311): per vertex totalAngle = 0.; per slice angle = fraction * 2. * pi, angle0 = totalAngle, boundaryX = llround(cos(angle0) *
 * 1048576.), boundaryY = llround(sin(angle0) * 1048576.), largeArc = angle > pi, totalAngle = angle0 + angle.  The cosines and
 * sines thereby stay out of the kernel, whose results are exact because the vectors are its inputs; 2^20 resolves two
 * subpixels at the largest radius.  Host only; the C library's cos and sin. */
int em2_pie_boundaries(uint32_t vertexCount, const uint64_t* sliceOffsets, const double* sliceFraction, int32_t* boundaryX,
                       int32_t* boundaryY, uint8_t* largeArc);

/* SignatureGraph::writeSvg (src/SignatureGraph.cpp:183-321) into a file, byte for byte for the same doubles and strings.  As
 * written: the maxima of the coordinates start at numeric_limits<double>::min(); viewBoxSize = 1.05 * boundingBoxSize /
 * zoomFactor; the vertices in the order of em2_order_by_count over cellCounts; the radius 0.03 * boundingBoxSize *
 * sqrt(double(cellCount) / double(maxCellCount)); a circle for a vertex of fewer than two slices ("black" for none), else per
 * slice a path with cos, sin, the large-arc flag angle > pi and the running totalAngle.  sliceOffsets NULL: no vertex has a
 * colour, every vertex is the black circle (what the reference's createSignatureGraph writes into SignatureGraph.svg).
 * sliceColors: sliceCount strings, each followed by a 0 byte.  svgParameters[4] = xCenter, yCenter, halfViewBoxSize, pixelSize,
 * the four fields the reference fills in.  Host only. */
int em2_signature_graph_write_svg(const char* fileName, uint32_t vertexCount, const double* x, const double* y, const uint64_t* cellCounts,
                                  uint64_t edgeCount, const uint32_t* v0, const uint32_t* v1, int hideEdges, double svgSizePixels,
                                  double xShift, double yShift, double zoomFactor, double vertexSizeFactor, double edgeThicknessFactor,
                                  const uint64_t* sliceOffsets, const char* sliceColors, uint64_t sliceColorsBytes,
                                  const double* sliceFraction, double* svgParameters);

/* ExpressionMatrixSubset + Lsh + findSimilarPairs4 in one call on host buffers (SURVEY.md 8(a) row a1 on the device:
 * src/ExpressionMatrixSubset.cpp:9-42 followed by src/Lsh.cpp:118-224 and src/ExpressionMatrixLsh.cpp:200-285): the
 * global CSR (CellExpressionCounts toc/data, global gene ids) restricted to the cells cellIds[0..cellCount) (NULL =
 * all cells in order) and to the genes with geneLocalIds[globalGeneId] != 0xffffffff (GeneSet-<name>-LocalIds), gene
 * ids remapped to those local ids; geneCount = size of the gene set = rows of `vectors`.  The restricted CSR never
 * exists on the host.  signatures may be NULL (not wanted); usedCount == NULL stops after the signatures
 * (computeLshSignatures), otherwise pairs / usedCount receive the SimilarPairs content as em2_find_similar_pairs4. */
int em2_subset_find_similar_pairs4(const uint64_t* globalToc, const em2_count* globalData, uint32_t globalCellCount,
                                   const uint32_t* cellIds, uint32_t cellCount, const uint32_t* geneLocalIds,
                                   uint32_t globalGeneCount, uint32_t geneCount, const double* vectors, uint32_t lshCount,
                                   uint64_t* signatures, uint32_t k, double similarityThreshold, em2_pair* pairs,
                                   uint32_t* usedCount);

/* ExpressionMatrix::findSimilarPairs5 (src/ExpressionMatrixLsh.cpp:355-496).  lshSliceLength must be in
 * [1,32] (the reference divides by zero for 0 and allocates 2^lshSliceLength vectors per slice). */
int em2_find_similar_pairs5(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                            double similarityThreshold, uint32_t lshSliceLength, uint64_t bucketOverflow,
                            em2_pair* pairs, uint32_t* usedCount);

/* ------------------------------------------------------------------------------------------------------
 * Device-resident entry points (multi-GPU sharding, benchmarking, callers that keep data in HBM).
 * ------------------------------------------------------------------------------------------------------ */

/* Bytes of device scratch em2_dev_compute_signatures needs. */
size_t em2_dev_compute_signatures_workspace(uint32_t cellCount, uint32_t lshCount);

/* Per-hyperplane-matrix auxiliary block (built once, reused for every shard / call): lshVectorsSums of
 * src/Lsh.cpp:137-144, the per-hyperplane maximum magnitude and a float copy of the matrix used by the screening
 * pass of em2_dev_compute_signatures. */
size_t em2_dev_vector_aux_bytes(uint32_t geneCount, uint32_t lshCount);
int em2_dev_prepare_vectors(const double* d_vectors, uint32_t geneCount, uint32_t lshCount, void* d_vectorAux,
                            void* stream);

/* As em2_compute_signatures, for the cellCount cells of a (shard of a) CSR in device memory.
 * d_vectorAux: the block em2_dev_prepare_vectors filled, or NULL.  With it (and lshCount a multiple of 4) most bits
 * are decided by a pass over the float copy of the hyperplanes under a rigorous error bound and only the undecided
 * 64-bit words are recomputed in the reference's sequential FP64 arithmetic; without it every bit is.  Both give
 * the same, reference-identical signatures. */
int em2_dev_compute_signatures(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount,
                               uint32_t geneCount, const double* d_vectors, const void* d_vectorAux,
                               uint32_t lshCount, uint64_t* d_signatures, void* d_workspace,
                               size_t workspaceBytes, void* stream);

/* Which FIRST tier the last em2_dev_compute_signatures call on this workspace ran (the result does not depend on it; the time
 * does -- DESIGN.md 3.2).  The call waits for the whole device (hipDeviceSynchronize: it has no stream argument), and the
 * workspace must be untouched since that call -- the tier is read from a word the projection leaves in it.  haveVectorAux:
 * whether that call was given d_vectorAux.
 *   EM2_TIER_EXACT           the reference's arithmetic on every bit (no auxiliary block, or lshCount no multiple of 4)
 *   EM2_TIER_FLOAT           the float copy of the hyperplanes under its error bound (lshCount no multiple of 64)
 *   EM2_TIER_FIXED16_FLOAT   the 16-bit fixed-point copy, products summed in floating point (some count is no small integer)
 *   EM2_TIER_FIXED16_INTEGER the 16-bit fixed-point copy, products summed exactly in 32-bit integers (every count an integer of
 *                            at most 15 bits, every cell's sum of |count| at most 65 535: expression COUNTS)                    */
enum { EM2_TIER_EXACT = 0, EM2_TIER_FLOAT = 1, EM2_TIER_FIXED16_FLOAT = 2, EM2_TIER_FIXED16_INTEGER = 3 };
int em2_dev_compute_signatures_tier(const void* d_workspace, uint32_t cellCount, uint32_t lshCount, int haveVectorAux, int* tier);

/* How far the tiers of that call got, read from the same workspace under the same conditions (it waits for the whole device, the
 * workspace must be untouched since the call); nothing is launched and nothing written on the device.  listed[3]:
 *   listed[0]  64-bit words the 16-bit tier listed for the word form of the float tier (several undecided bits)
 *   listed[1]  64-bit words the 16-bit tier listed by their single undecided bit, for the per-bit form of the float tier
 *   listed[2]  list entries left to the exact arithmetic: words behind the 16-bit and float tiers; where the float copy is the
 *              first tier, one entry per (cell, word) at lshCount no multiple of 32 and one per (cell, 32-bit slice) otherwise
 * Zeros for a tier the width does not have (listed[0], listed[1] at lshCount no multiple of 64) and all zeros when the call
 * had no auxiliary block or lshCount is no multiple of 4 (the exact arithmetic ran alone, without a list). */
int em2_dev_compute_signatures_listed(const void* d_workspace, uint32_t cellCount, uint32_t lshCount, int haveVectorAux, uint32_t* listed);

/* Bytes of device scratch em2_dev_find_similar_pairs4 needs for rowCount rows. */
size_t em2_dev_find_similar_pairs4_workspace(uint32_t cellCount, uint32_t rowCount, uint32_t lshCount,
                                             uint32_t k);

/* ExpressionMatrixSubset on device-resident arrays (src/ExpressionMatrixSubset.cpp:9-42), two steps because the size
 * of the result is not known beforehand: _count writes d_toc[0..cellCount] (offsets of the restricted CSR, d_toc[cellCount]
 * = its entry count, read it back to size d_data), _fill writes the entries.  d_cellIds NULL = all cells in order. */
size_t em2_dev_subset_workspace(uint32_t cellCount);
int em2_dev_subset_count(const uint64_t* d_globalToc, const em2_count* d_globalData, const uint32_t* d_cellIds,
                         uint32_t cellCount, const uint32_t* d_geneLocalIds, uint32_t globalGeneCount, uint64_t* d_toc,
                         void* d_workspace, size_t workspaceBytes, void* stream);
int em2_dev_subset_fill(const uint64_t* d_globalToc, const em2_count* d_globalData, const uint32_t* d_cellIds,
                        uint32_t cellCount, const uint32_t* d_geneLocalIds, uint32_t globalGeneCount, const uint64_t* d_toc,
                        em2_count* d_data, void* stream);

/* Which form of the scan em2_dev_find_similar_pairs4 runs for this shape -- information for benchmarks and logs, the
 * results are identical.  0: every row of the launch is compared with every column (cellCount*rowCount ordered
 * comparisons).  1: symmetric form, used when one launch holds all rows of a large problem: every unordered pair is
 * evaluated once, as in the reference's own loop (src/ExpressionMatrixLsh.cpp:218-263), and offered to both cells. */
int em2_dev_find_similar_pairs4_form(uint32_t cellCount, uint32_t rowCount);

/* The same question with the signature width: for 129..2048 bits the symmetric form contracts its pairs as FP4 dot
 * products on the matrix cores (3; up to 1024 bits 0 / 1 operands, popcount(a & b) - (popcount(a) + popcount(b)) / 2 =
 * -mismatches / 2; above, +-1 operands, 2048 - 2 * mismatches; both exact in f32)
 * and starts at 32768 cells instead of 131072.  A launch that is not symmetric -- a shard of the rows, SURVEY 8(e)'s
 * partitioning across GPUs -- takes the rows form on the matrix cores (4) from 2^31 (row, column) pairs on: every row walks
 * all columns in ascending order, which is the per-cell contract of src/ExpressionMatrixLsh.cpp:200-285 as it stands.
 * The last_launch query below reports what actually ran. */
int em2_dev_find_similar_pairs4_form_for(uint32_t cellCount, uint32_t rowCount, uint32_t lshCount);

/* Facts about the calling thread's last em2_dev_find_similar_pairs4 launch, for benchmarks: values[0] form (as above),
 * [1] duration in ms of the scan kernel proper when the launcher measured it with HIP events on the launch stream
 * (symmetric form, which synchronises anyway), else -1, [2] (64-row wave, column) steps executed, [3] symmetric
 * form: inbox entries sorted and replayed, [4] column segments, [5] cells whose rows scanned all columns, [6] pairs
 * contracted on the matrix cores and [7] the duration in ms of that kernel alone (form 3, the matrix-core form of the
 * symmetric scan: FP4 contraction, signatures zero-extended to 1024 or 2048 bits), [8] the shader clock in GHz that
 * kernel ran at (sums over its blocks of s_memtime and s_memrealtime ticks; 0 when unknown). */
int em2_dev_find_similar_pairs4_last_launch(double* values, uint32_t valueCount);


/* findSimilarPairs4 for the rows [rowBegin,rowEnd) of the cell set against all cellCount cells: the shard
 * one rank owns.  d_signatures holds ALL cellCount signatures (after the all-gather).  d_pairs has
 * (rowEnd-rowBegin)*k slots and d_usedCount (rowEnd-rowBegin) entries, indexed by row-rowBegin.
 * The first call for a given (lshCount, similarityThreshold) on a device builds and caches small lookup
 * tables (one synchronous allocation + copy); later calls only enqueue kernels. */
int em2_dev_find_similar_pairs4(const uint64_t* d_signatures, uint32_t cellCount, uint32_t rowBegin,
                                uint32_t rowEnd, uint32_t lshCount, uint32_t k, double similarityThreshold,
                                em2_pair* d_pairs, uint32_t* d_usedCount, void* d_workspace,
                                size_t workspaceBytes, void* stream);

/* findSimilarPairs7 on device-resident signatures for the cells [rowBegin,rowEnd) (buckets over all cells; rows
 * shard over ranks like em2_dev_find_similar_pairs5).  sliceLengths is a host array.  Allocates its own scratch and
 * synchronises the stream. */
int em2_dev_find_similar_pairs7(const uint64_t* d_signatures, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd,
                                uint32_t lshCount, uint32_t k, double similarityThreshold, const int32_t* sliceLengths,
                                uint32_t sliceLengthCount, uint32_t maxCheck, uint32_t log2BucketCount, em2_pair* d_pairs,
                                uint32_t* d_usedCount, void* stream);

/* findSimilarPairs6 on device-resident signatures for the cells [rowBegin,rowEnd) (the sorted permutation tables
 * always cover all cells; rows shard over ranks like em2_dev_find_similar_pairs5).  Allocates its own scratch and
 * synchronises the stream. */
int em2_dev_find_similar_pairs6(const uint64_t* d_signatures, uint32_t cellCount, uint32_t rowBegin, uint32_t rowEnd,
                                uint32_t lshCount, uint32_t k, double similarityThreshold, uint32_t permutationCount,
                                uint32_t searchCount, uint32_t permutedBitCount, int32_t seed,
                                em2_pair* d_pairs, uint32_t* d_usedCount, void* stream);

/* em2_find_similar_pairs0 on a device-resident CSR for the cells [rowBegin,rowEnd) against all cells: d_pairs
 * [(rowEnd-rowBegin)][k] and the three per-cell arrays [rowEnd-rowBegin], indexed by row - rowBegin (rows shard over
 * ranks like em2_dev_find_similar_pairs5; every cell's result is independent of the others).  d_workspace holds
 * em2_dev_find_similar_pairs0_workspace(cellCount, rowEnd-rowBegin, geneCount, k) bytes.  The gene ids are checked on
 * the device before any kernel indexes with them.  Synchronises the stream. */
size_t em2_dev_find_similar_pairs0_workspace(uint32_t cellCount, uint32_t rowCount, uint32_t geneCount, uint32_t k);
int em2_dev_find_similar_pairs0(const uint64_t* d_toc, const em2_count* d_data, uint32_t cellCount, uint32_t geneCount,
                                uint32_t rowBegin, uint32_t rowEnd, uint32_t k, double similarityThreshold, em2_pair* d_pairs,
                                uint32_t* d_usedCount, uint32_t* d_lowestSimilarityIndex, float* d_lowestSimilarity,
                                void* d_workspace, size_t workspaceBytes, void* stream);

/* ---- findSimilarPairs4 across GPUs with every unordered pair evaluated once (one process per GPU) ----
 * The 64-cell blocks of the problem are dealt round-robin to the ranks (block g: rank g % world).  Every rank holds
 * ALL signatures (after the all-gather of the projection shards) and calls the four phases in order with the same
 * arguments; between the phases the CALLER runs the collectives on views of the workspace:
 *     phase 0;  all_reduce(MAX) of snap = int32[cellCount] at snapOffset
 *     phase 1;  all_reduce(MAX) of snap
 *     phase 2;  em2_dev_fsp4_sharded_status -> own entry count; all ranks agree on maxUsed = max of the counts, fill
 *               pool[used, maxUsed) with ~0 (pool = uint64[poolCapacity] at poolOffset), all_gather pool[0, maxUsed)
 *               into gathered = uint64[world*maxUsed] at gatheredOffset
 *     phase 3 with gatheredCount = world*maxUsed
 * or, when world is a power of two, exchanging only what each rank needs:
 *     phase 2;  status -> used;  phase 4 with gatheredCount = used: the pool entries grouped by the rank that owns their
 *               target cell ((key >> ownerShift) & (world-1)) in sorted = uint64[..] at sortedOffset; all_to_all of those
 *               groups into gathered; phase 3 with gatheredCount = entries received
 * d_pairs [cellCount][k] and d_usedCount [cellCount] are indexed by GLOBAL cell id; phase 3 fills the rows of the
 * cells this rank owns.  If any rank reports overflow the result is unusable and the caller falls back to
 * em2_dev_find_similar_pairs4 on row shards.  em2_dev_fsp4_sharded_plan: values[0] eligible (0: shape too small, use
 * the row-shard call), [1] workspace bytes (256-byte aligned allocation), [2] snapOffset, [3] poolOffset,
 * [4] poolCapacity, [5] gatheredOffset, [6] gatheredCapacity, [7] prefix cells, [8] blocks owned, [9] blocks,
 * [10] sortedOffset, [11] ownerShift.
 * No reference counterpart (the reference is single-threaded); results are those of src/ExpressionMatrixLsh.cpp:155-290. */
int em2_dev_fsp4_sharded_plan(uint32_t cellCount, uint32_t lshCount, uint32_t k, uint32_t rank, uint32_t world,
                              uint64_t* values, uint32_t valueCount);
int em2_dev_fsp4_sharded_phase(int phase, const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint32_t k,
                               double similarityThreshold, uint32_t rank, uint32_t world, em2_pair* d_pairs,
                               uint32_t* d_usedCount, void* d_workspace, size_t workspaceBytes, uint64_t gatheredCount,
                               void* stream);
int em2_dev_fsp4_sharded_status(uint32_t cellCount, uint32_t k, uint32_t rank, uint32_t world, const void* d_workspace,
                                void* stream, uint64_t* usedEntries, uint32_t* overflow);

/* ---- findSimilarPairs4 across the GPUs of a node from C or C++ (csrc/em2_dist.hip) ----
 * One process per GPU.  Every rank calls with the same arguments and its own shard of the signatures -- the cells
 * [rank * shard, min(cellCount, (rank + 1) * shard)), shard = ceil(cellCount / world), the contiguous ranges of north_star --
 * and ends with the SimilarPairs rows of exactly those cells.  The function issues every collective itself:
 *   rows form       all_gather of the signature shards, then em2_dev_find_similar_pairs4 on the rank's rows;
 *   symmetric form  (large problems; every unordered pair once across the ranks) all_gather, phases 0-3 of
 *                   em2_dev_fsp4_sharded_phase with two all_reduce(MAX) of the snapshots, one small all_gather by which the
 *                   ranks agree on entry counts and overflow, the all_to_all of the deferred candidates (all_gather when
 *                   world is not a power of two), and an all_to_all that moves the finished rows from the block-cyclic
 *                   owners to the contiguous ranges.  A pool overflow on any rank sends all ranks to the rows form.
 * em2_dist_find_similar_pairs4_form: 2 if a problem of this shape takes the symmetric form, else 0 (EM2_SHARDED_SCAN=0 and
 * EM2_SHARDED_MIN_CELLS as in expressionmatrix2_amd/sharded.py, whose DevicePipeline is this choreography in Python).
 *   d_localSignatures  [shard][words] device: the rank's signatures (the last rank's unused tail is ignored)
 *   d_allSignatures    [shard * world][words] device: receives all signatures (rows [0, cellCount) are the cells)
 *   d_pairs / d_usedCount  [rows][k] / [rows] device, rows = the rank's range
 *   d_workspace        em2_dist_find_similar_pairs4_workspace(...) bytes, device
 *   stageMs            NULL, or EM2_DIST_MS_COUNT doubles that receive the wall time per kind of stage; asking for them
 *                      synchronises the stream after every stage (measurements), NULL leaves the call asynchronous up to
 *                      the read-backs the exchange needs
 * em2_dist_find_similar_pairs4 takes an RCCL communicator (ncclComm_t, passed as void*: this header does not include
 * rccl.h).  RCCL is bound at run time -- the nccl* symbols already in the process (the library that made the communicator),
 * else librccl.so.1 -- so libem2lsh.so has no link-time dependency on it.  em2_dist_find_similar_pairs4_with takes the
 * transport as a table instead (MPI, a test harness, ...): every function works on DEVICE buffers, is called by all ranks
 * in the same order, is ordered after earlier work on `stream` and before later work on it, and returns 0 or an error.
 * all_gather's send buffer may be the rank's own slot of the receive buffer.  all_to_all_v gets byte counts and byte
 * offsets per peer (host arrays of `world` entries).
 * A HIP or transport error on one rank ends that rank's call with an error while the others may wait in a collective:
 * abort the communicator (ncclCommAbort), as in any RCCL program.  No reference counterpart (the reference is one thread). */
typedef struct em2_collectives {
    void* context;
    int world;
    int rank;
    int (*all_gather)(void* context, const void* d_send, void* d_recv, size_t bytesPerRank, void* stream);
    int (*all_reduce_max_i32)(void* context, void* d_buffer, size_t count, void* stream);
    int (*all_to_all_v)(void* context, const void* d_send, const uint64_t* sendBytes, const uint64_t* sendOffsets,
                        void* d_recv, const uint64_t* recvBytes, const uint64_t* recvOffsets, void* stream);
} em2_collectives;
#define EM2_DIST_MS_GATHER_SIGNATURES 0
#define EM2_DIST_MS_SCAN 1
#define EM2_DIST_MS_ALL_REDUCE 2
#define EM2_DIST_MS_EXCHANGE 3
#define EM2_DIST_MS_REDISTRIBUTE 4
#define EM2_DIST_MS_COUNT 5
size_t em2_dist_find_similar_pairs4_workspace(uint32_t cellCount, uint32_t lshCount, uint32_t k, uint32_t rank, uint32_t world);
int em2_dist_find_similar_pairs4_form(uint32_t cellCount, uint32_t lshCount, uint32_t k, uint32_t world);
int em2_dist_find_similar_pairs4(void* ncclCommunicator, const uint64_t* d_localSignatures, uint32_t cellCount, uint32_t lshCount,
                                 uint32_t k, double similarityThreshold, uint64_t* d_allSignatures, em2_pair* d_pairs,
                                 uint32_t* d_usedCount, void* d_workspace, size_t workspaceBytes, void* stream, double* stageMs);
int em2_dist_find_similar_pairs4_with(const em2_collectives* collectives, const uint64_t* d_localSignatures, uint32_t cellCount,
                                      uint32_t lshCount, uint32_t k, double similarityThreshold, uint64_t* d_allSignatures,
                                      em2_pair* d_pairs, uint32_t* d_usedCount, void* d_workspace, size_t workspaceBytes,
                                      void* stream, double* stageMs);

/* Synchronises `stream` and reports whether the last em2_dev_find_similar_pairs4 on this workspace completed: the
 * scan hands per-row state from one column segment to the next between waves, and a hand-off wait that exceeds
 * ~4 s raises an error word instead of hanging the GPU (never observed).  rowCount and k as in that call. */
int em2_dev_find_similar_pairs4_status(const void* d_workspace, uint32_t rowCount, uint32_t k, void* stream);

/* findSimilarPairs5 for the cells [rowBegin,rowEnd) of the cell set (the bucket tables are built over all
 * cellCount signatures, which every rank holds after the all-gather).  Unlike the other dev entry points this one
 * sizes its scratch from the data (bucket sizes are only known after the sort), so it allocates and frees device
 * memory itself and returns after synchronising the stream. */
int em2_dev_find_similar_pairs5(const uint64_t* d_signatures, uint32_t cellCount, uint32_t rowBegin,
                                uint32_t rowEnd, uint32_t lshCount, uint32_t k, double similarityThreshold,
                                uint32_t lshSliceLength, uint64_t bucketOverflow, em2_pair* d_pairs,
                                uint32_t* d_usedCount, void* stream);

/* Facts about the calling thread's last em2_dev_find_similar_pairs5 / em2_find_similar_pairs5, for benchmarks:
 * values[0] candidate ids gathered from the buckets (duplicates and the cell itself included: each costs the filter
 * one look at the sorted list, each distinct one a gather of 8*W signature bytes), [1] cells queried, [2] slices
 * (lshCount / lshSliceLength, src/ExpressionMatrixLsh.cpp:355), [3] batches, [4] / [5] ms of the candidate filter and
 * of the selection, summed over the batches (HIP events on the launch stream), [6] the DISTINCT candidates of all cells
 * (the sizes of the duplicate-free unions, the cell itself included): the signatures the filter actually gathers.
 * Which forms ran (facts the host holds; nothing is measured for them): [7] the candidate union, 1 = bitmap in LDS, 0 = gather +
 * segmented sort (more than 256 slices); [8] passes of the bitmap over the cell ids, ceil(cellCount / values[9]), 0 in the sort
 * form; [9] cell ids per pass; [10] the candidate filter: 0 one lane per candidate, 1 cooperative 8-byte loads, 2..8 the
 * 16-byte forms <T units per lane, LPC lanes per candidate (0 = decided at run time), FULL> = 2 <4,4,true>, 3 <1,16,false>,
 * 4 <1,8,false>, 5 <1,0,false>, 6 <2,16,true>, 7 <2,16,false>, 8 <2,0,false>; [11] the selection, 1 = packed tiers ({key,
 * position} in four bytes: k <= 2048), 0 = tiers of whole entries.  Entries beyond the last one defined are 0. */
int em2_dev_find_similar_pairs5_last_launch(double* values, uint32_t valueCount);

/* findSimilarPairs5 keeps its device scratch (bucket tables, candidate ids, candidate lists: about 10 GB at a million cells x
 * 2048 bits) between calls of the process, and em2_subset_find_similar_pairs4 the device copy of its result and its scan
 * workspace (12 GB at a million cells: it starts with room for 512 deferred candidates per cell and takes the 19 GB of the
 * device-level call once a launch of the process has overflowed that), because allocating gigabytes costs anything between
 * 2 ms and 2.7 s per call depending on the state of the host; at most EM2_SCRATCH_CACHE_MB megabytes are kept (default: a
 * sixteenth of the device's memory -- 18 GB of an MI355X's 288 --, the oldest blocks making room for newer ones; 0 = none).
 * This call frees what is kept.  The reference has no counterpart (its tables are std::vectors of the call,
 * src/ExpressionMatrixLsh.cpp:377-389). */
void em2_dev_release_scratch(void);

/* ------------------------------------------------------------------------------------------------------
 * SURVEY.md 8(f), first "next" row: the consumer of SimilarPairs.
 * ------------------------------------------------------------------------------------------------------ */

/* CellGraph::CellGraph (src/CellGraph.cpp:33-117; reached from ExpressionMatrix::createCellGraph,
 * src/ExpressionMatrix.cpp:1795-1845): the edges of the k-NN cell similarity graph in the order the reference adds
 * them.  Vertex v is the v-th cell of graphCellSet (the order of add_vertex).  pairs / usedCount / k are the content
 * of a SimilarPairs object whose cell set (sorted global ids) is similarPairsCellSet.  maxConnectivity 0 means no
 * limit, as in the reference (the size test at :101 follows a push_back).  The three output arrays need room for
 * graphCellCount*min(maxConnectivity ? maxConnectivity : k, k) edges; *edgeCount receives the number written.
 * Host buffers. */
int em2_cell_graph_edges(const em2_pair* pairs, const uint32_t* usedCount, uint32_t similarPairsCellCount, uint32_t k,
                         const uint32_t* similarPairsCellSet, const uint32_t* graphCellSet, uint32_t graphCellCount,
                         double similarityThreshold, uint32_t maxConnectivity, uint32_t* edgeVertex0,
                         uint32_t* edgeVertex1, float* edgeSimilarity, uint64_t* edgeCount);

/* The same with the SimilarPairs content still on the device (d_pairs / d_usedCount as em2_dev_find_similar_pairs4
 * left them; the cell sets are host arrays as above; the three edge arrays may be host OR device memory): the consumer of a
 * device-resident findSimilarPairs4 does not move 8 * k * cells bytes over PCIe twice, and with device edge arrays handed on
 * to em2_cell_graph_label_propagation (which takes host or device edge arrays as well) the edges never leave the device. */
int em2_dev_cell_graph_edges(const em2_pair* d_pairs, const uint32_t* d_usedCount, uint32_t similarPairsCellCount, uint32_t k,
                             const uint32_t* similarPairsCellSet, const uint32_t* graphCellSet, uint32_t graphCellCount,
                             double similarityThreshold, uint32_t maxConnectivity, uint32_t* edgeVertex0,
                             uint32_t* edgeVertex1, float* edgeSimilarity, uint64_t* edgeCount);

/* ExpressionMatrix::analyzeLsh (src/ExpressionMatrixLsh.cpp:1244-1367; Python: src/PythonModule.cpp:940-944): the
 * quality of the LSH similarity against the exact one, over every unordered pair of cells of an expression matrix
 * subset.  SURVEY.md 8(f).
 *   toc / data      : the subset's counts (what em2_matrix_subset / em2_dev_subset_* produce: local gene ids ascending)
 *   geneCount       : size of the gene set -- the n of the correlation coefficient (src/ExpressionMatrixSubset.cpp:115)
 *   signatures      : the cells' LSH signatures (em2_compute_signatures), lshCount bits each
 *   globalCellIds   : the cell set (column 3 and 4 of the pairs csv)
 *   seed            : seeds the mt19937 that downsamples the pairs csv (one draw per pair, in pair order)
 *   pairsCsvPath / statisticsCsvPath : the reference writes "Lsh-analysis.csv" and "LSH-analysis-statistics.csv" into
 *                     the working directory; statisticsCsvPath may be NULL
 *   sum0 / sum1 / sum2 (each 200 entries, may be NULL): per bin of exact similarity the number of pairs, the sum of
 *                     (lsh - exact) and the sum of its square, accumulated in the reference's pair order
 *   exactSimilarity / lshSimilarity (cellCount * (cellCount - 1) / 2 entries, may be NULL): the values per pair
 * The scalar products of the pairs and the mismatch counts are computed on the device (bit-identical to the
 * reference's merge loop: float products, double sum, ascending gene); what the reference's pair order defines (the
 * bins' double sums, the random draws, the csv) is walked on the host in that order.  Bit-exact in all outputs.
 * Errors: EM2_ERROR_RUNTIME "bin < binCount" where the reference's CZI_ASSERT (:1322) throws (a pair with exact
 * similarity 1, or without variance); the files are then incomplete, as the reference's are. */
int em2_analyze_lsh(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                    const uint64_t* signatures, uint32_t lshCount, const uint32_t* globalCellIds, uint32_t seed,
                    double csvDownsample, const char* pairsCsvPath, const char* statisticsCsvPath,
                    uint64_t* sum0, double* sum1, double* sum2, double* exactSimilarity, double* lshSimilarity);


/* ExpressionMatrix::analyzeSimilarPairs after its lookups (src/ExpressionMatrixLsh.cpp:71-148) on a subset's CSR (toc
 * from 0) and the content of a stored SimilarPairs object (pairs[cellCount][k], usedCount[cellCount], local ids): the
 * exact similarity of every stored pair on the device, then in the reference's order (cell 0 ascending, stored order)
 * delta = stored - exact into 200 bins of exact similarity, one draw per pair of mt19937(231) / uniform_01 against
 * csvDownsample, and the csv line (GlobalCellId0,GlobalCellId1,ExactSimilarity,StoredSimilarity) to pairsCsvPath;
 * statisticsCsvPath gets Similarity,Bias,Rms for bins with at least 2 pairs.  sum0/sum1/sum2 [200] may be NULL.
 * CZI_ASSERT(bin < binCount) (:111) is EM2_ERROR_RUNTIME. */
int em2_analyze_similar_pairs(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                              const em2_pair* pairs, const uint32_t* usedCount, uint32_t k, const uint32_t* globalCellIds,
                              double csvDownsample, const char* pairsCsvPath, const char* statisticsCsvPath,
                              uint64_t* sum0, double* sum1, double* sum2);

/* CellGraph::labelPropagationClustering (src/CellGraph.cpp:443-612, ClusterTable src/CellGraph.hpp:50-121; reached
 * from ExpressionMatrix::createClusterGraph, src/ExpressionMatrix.cpp:2145-2149) over the graph em2_cell_graph_edges
 * built.  SURVEY.md 8(f) row 2.  vertexCellIds[v] is the cell id of vertex v, in add_vertex order with removed
 * isolated vertices left out; edges index that array and are in add_edge order.  clusterIds[v] receives the cluster
 * of vertex v after the reference's renumbering (0 = largest; equal sizes by decreasing original label).
 * *iterationCount (may be NULL) receives the number of iterations that ran.  The reference's schedule is serial by
 * definition (each update reads labels written earlier in the same std::shuffle(std::mt19937(seed)) order, and
 * the float weights accumulate in that order); the device runs it with a schedule that reproduces exactly those labels
 * (csrc/em2_cluster.hip).  Host buffers.  em2_dev_cell_graph_label_propagation takes the three edge arrays in DEVICE memory,
 * as em2_dev_cell_graph_edges left them when given device output arrays (they are not validated again): with the pairs of
 * em2_dev_find_similar_pairs4 the chain findSimilarPairs4 -> createCellGraph -> labelPropagationClustering then keeps pairs
 * and edges on the device from end to end; vertexCellIds and clusterIds stay host arrays. */
int em2_cell_graph_label_propagation(const uint32_t* vertexCellIds, uint32_t vertexCount, const uint32_t* edgeVertex0,
                                     const uint32_t* edgeVertex1, const float* edgeSimilarity, uint64_t edgeCount,
                                     uint64_t seed, uint64_t stableIterationCountThreshold,
                                     uint64_t maxIterationCount, uint32_t* clusterIds, uint64_t* iterationCount);
int em2_dev_cell_graph_label_propagation(const uint32_t* vertexCellIds, uint32_t vertexCount, const uint32_t* d_edgeVertex0,
                                     const uint32_t* d_edgeVertex1, const float* d_edgeSimilarity, uint64_t edgeCount,
                                     uint64_t seed, uint64_t stableIterationCountThreshold,
                                     uint64_t maxIterationCount, uint32_t* clusterIds, uint64_t* iterationCount);

/* ------------------------------------------------------------------------------------------------------
 * The rest of ExpressionMatrix::createClusterGraph (src/ExpressionMatrix.cpp:2087-2185) after the label propagation:
 * ClusterGraph (src/ClusterGraph.cpp:59-386).  csrc/em2_cluster_graph.hip.  Host buffers.
 * ------------------------------------------------------------------------------------------------------ */

/* ExpressionMatrix::computeAverageExpression with NormalizationMethod::L2 (src/ExpressionMatrix.cpp:1179-1245, and
 * computeExpressionVector :1253-1296) for clusterCount lists of cells at once.  toc / data: the counts restricted to the gene
 * set (what em2_matrix_subset produces: local gene ids strictly ascending within a cell, below geneCount).  Cluster c holds the
 * cells (rows of the CSR) clusterCells[clusterOffsets[c] .. clusterOffsets[c+1]), clusterOffsets[0] = 0; their ORDER is the
 * order of the reference's double additions and is kept.  averages[clusterCount][geneCount].  Per cell the norm is the double
 * sum of the float products c*c in stored order, factor = float(1/sqrt(sum)), every count float(c*factor); per cluster and gene
 * the double sum over the cells in list order, times 1/double(cell count); then sum += a*a over the genes ascending and
 * a *= 1/sqrt(sum).  No operation is contracted.  An empty cluster, or cells without counts, give the reference's NaN / inf.
 * Errors: EM2_ERROR_INVALID_ARGUMENT for gene ids out of range or not ascending and rows that do not exist; EM2_ERROR_HIP
 * ("out of memory", with the sizes) when the table clusterCount * geneCount * 8 bytes and the sort of the listed cells' counts
 * (24 bytes each) do not fit into the device's free memory. */
int em2_cluster_average_expression(const uint64_t* toc, const em2_count* data, uint32_t cellCount, uint32_t geneCount,
                                   const uint32_t* clusterCells, const uint64_t* clusterOffsets, uint32_t clusterCount,
                                   double* averages);

/* ClusterGraph::computeSimilarities (src/ClusterGraph.cpp:154-169): similarity[e] = regressionCoefficient
 * (src/regressionCoefficient.cpp:10-42) of the rows edgeCluster0[e] and edgeCluster1[e] of averages[clusterCount][geneCount]:
 * the five double sums over the genes ascending, every product rounded before its addition (sx and sxx once per cluster: the
 * order, hence the bits, are those of the per-edge loop), then n*sxy - sx*sy over sqrt((n*sxx - sx*sx) * (n*syy - sy*sy)). */
int em2_cluster_similarities(const double* averages, uint32_t clusterCount, uint32_t geneCount, const uint32_t* edgeCluster0,
                             const uint32_t* edgeCluster1, uint64_t edgeCount, double* similarity);

/* ExpressionMatrix::createClusterGraph from the ClusterGraph constructor on (src/ExpressionMatrix.cpp:2153-2181):
 *   ClusterGraph::ClusterGraph (src/ClusterGraph.cpp:61-120)  a vertex per distinct label at its first occurrence in vertex
 *       order, cells appended in vertex order, an edge per unordered pair of distinct clusters joined by a cell-graph edge;
 *   mergeVertices (:174-270)   averages and similarities, connected components over edges with similarity >
 *       similarityThresholdForMerge; the first vertex of a component survives, the others' cells are appended to it in vertex
 *       order, their edges go with them (they are NOT transferred);
 *   removeSmallVertices (:304-319)   fewer than minClusterSize cells: removed, cells appended to unclusteredCells;
 *   averages and similarities again, removeWeakEdges (:324-336: similarity < similarityThreshold), makeKnn (:342-386: an edge
 *       stays if it is among the k most similar of at least one of its vertices);
 *   renumberClusters (:276-299)   std::sort of (vertex, uint32 size) in vertex order by size descending -- not stable; the
 *       host's own std::sort runs on the same sequence.
 * Inputs: the counts as for em2_cluster_average_expression with rowCount rows; vertexRows[v] = the row of cell-graph vertex v
 * (NULL: row v); the cell graph's edges as vertex pairs in add_edge order; labels[v] = the clusterId of vertex v (what
 * em2_cell_graph_label_propagation returned).  Label propagation itself is not run here.
 * Two places the reference does not pin: edges of one vertex with exactly equal similarity are ordered by makeKnn's sort by
 * their Boost descriptors (addresses) -- here the edge created later by the constructor ranks higher; and a NaN similarity
 * (a cluster without variance or with an all-zero average) that is left when makeKnn starts makes that sort undefined --
 * EM2_ERROR_RUNTIME.
 * The result is an object: em2_cluster_graph_sizes, then em2_cluster_graph_get into arrays of those sizes (any may be NULL):
 *   clusterIds[clusterCount]        the final cluster id of every surviving vertex, in vertex order
 *   cellOffsets[clusterCount + 1], cells[clusteredCellCount]   ClusterGraphVertex::cells as cell-graph vertex indices
 *   unclusteredCells[unclusteredCellCount]                     ClusterGraph::unclusteredCells, likewise
 *   averages[clusterCount][geneCount]                          ClusterGraphVertex::averageGeneExpression
 *   edgeCluster0 / edgeCluster1 / edgeSimilarity[edgeCount]    the surviving edges as final cluster ids (source, target as
 *                                                              created), in the order of their creation
 * em2_cluster_graph_facts (benchmarks): values[0] seconds of the call, [1] of both average computations, [2] of both
 * similarity computations (the rest is host bookkeeping and the upload), [3] vertices and [4] edges before the merge. */
typedef struct em2_cluster_graph em2_cluster_graph;
int em2_cluster_graph_create(const uint64_t* toc, const em2_count* data, uint32_t rowCount, uint32_t geneCount,
                             const uint32_t* vertexRows, uint32_t vertexCount, const uint32_t* edgeVertex0,
                             const uint32_t* edgeVertex1, uint64_t edgeCount, const uint32_t* labels, uint64_t minClusterSize,
                             uint64_t k, double similarityThreshold, double similarityThresholdForMerge, em2_cluster_graph** graph);
int em2_cluster_graph_sizes(const em2_cluster_graph* graph, uint32_t* clusterCount, uint32_t* geneCount, uint64_t* clusteredCellCount,
                            uint64_t* unclusteredCellCount, uint64_t* edgeCount);
int em2_cluster_graph_get(const em2_cluster_graph* graph, uint32_t* clusterIds, uint64_t* cellOffsets, uint32_t* cells,
                          uint32_t* unclusteredCells, double* averages, uint32_t* edgeCluster0, uint32_t* edgeCluster1,
                          double* edgeSimilarity);
int em2_cluster_graph_facts(const em2_cluster_graph* graph, double* values, uint32_t valueCount);
void em2_cluster_graph_free(em2_cluster_graph* graph);

/* ------------------------------------------------------------------------------------------------------
 * The signature graph and the signature diagnostics: the consumers of the Lsh-<name> objects that group the cells by equal
 * signature.  csrc/em2_signature_graph.hip, DESIGN.md 3.13.  Integer work: every output is bit-exact.
 * A signature is wordCount = (lshCount - 1) / 64 + 1 words, the first bit the most significant of word 0, the bits at or beyond
 * lshCount zero (src/BitSet.hpp:46-62; EM2_ERROR_INVALID_ARGUMENT where one is set).  lshCount above 65536:
 * EM2_ERROR_UNSUPPORTED.
 * The reference is only defined for lshCount <= 64: BitSet's copy constructor and operator= allocate ONE word
 * (src/BitSet.hpp:184, :200), and both SignatureGraph::createEdges (src/SignatureGraph.cpp:37) and the comparator of
 * analyzeLshSignatures' sort (src/ExpressionMatrixLsh.cpp:1435) go through them.  For more words this library continues the same
 * contract: the order of std::lexicographical_compare over the words, one-bit neighbours across all words.
 * ------------------------------------------------------------------------------------------------------ */

/* ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150) after its lookups and
 * SignatureGraph::createEdges (src/SignatureGraph.cpp:23-48):
 *   groups     all cells with the same signature, in the order of the reference's std::map<BitSetPointer, vector<CellId>>
 *              (:72-75; src/BitSet.hpp:157-160: ascending by word 0, then word 1, ... as unsigned integers), the cell ids of
 *              a group ascending; *distinctCount of them ("Found ... populated signatures", :76);
 *   vertices   the groups of at least minCellCount cells (:118-120, a size_t comparison: 0 and 1 keep everything), numbered
 *              from 0 in that order;
 *   edges      for v0 ascending and bit 0 .. lshCount-1 ascending: where the bit is 0 in v0's signature and a VERTEX v1 has
 *              that signature with the bit set, the edge (v0, v1) -- v1 > v0 always; Boost's add_edge order.
 * signatures: [cellCount][wordCount], host memory (em2_dev_signature_graph_create: device memory).  cellCount 0 is an
 * error, as the reference's empty cell set is.  The result is an object: em2_signature_graph_sizes, then
 * em2_signature_graph_get into arrays of those sizes (any may be NULL):
 *   vertexSignatures[vertexCount][wordCount], cellOffsets[vertexCount + 1], cells[cellCount of the sizes] (ids local to the
 *   cell set, i.e. row numbers of `signatures`), edgeVertex0 / edgeVertex1[edgeCount].
 * A graph without vertices (minCellCount above every group's size) is a valid result.
 * Not built: SignatureGraph.svg and the layout behind it (:145-147), the colouring by meta data, the progress lines. */
typedef struct em2_signature_graph em2_signature_graph;
int em2_signature_graph_create(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount,
                               em2_signature_graph** graph);
int em2_dev_signature_graph_create(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount,
                                   em2_signature_graph** graph);
int em2_signature_graph_sizes(const em2_signature_graph* graph, uint64_t* distinctCount, uint32_t* vertexCount, uint32_t* wordCount,
                              uint64_t* cellCount, uint64_t* edgeCount);
int em2_signature_graph_get(const em2_signature_graph* graph, uint64_t* vertexSignatures, uint64_t* cellOffsets, uint32_t* cells,
                            uint32_t* edgeVertex0, uint32_t* edgeVertex1);
void em2_signature_graph_free(em2_signature_graph* graph);

/* The counts of Lsh::writeSignatureStatistics (src/Lsh.cpp:279-303): setCount[i] = the cells with bit i set, i < lshCount.
 * Host signatures (em2_dev_lsh_signature_statistics: device memory); setCount is a host array in both. */
int em2_lsh_signature_statistics(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount);
int em2_dev_lsh_signature_statistics(const uint64_t* d_signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount);

/* ExpressionMatrix::analyzeLshSignatures (src/ExpressionMatrixLsh.cpp:1372-1474) from its signatures on: three files in
 * `directory` (NULL or "": the working directory, where the reference writes them).
 *   Signatures.csv              a line per distinct signature, x for a set bit and _ for a clear one (BitSetPointer::getString,
 *                               src/BitSet.hpp:124-136), a comma, the number of cells; ordered by std::sort with
 *                               OrderPairsBySecondGreater (src/orderPairs.hpp:56-62) over the groups in map order -- not
 *                               stable: this library's own std::sort runs on that sequence, as for renumberClusters;
 *   Histogram.csv               for every group size i that occurs, ascending: i,frequency,frequency*i,running sum (no header);
 *   LshSignatureStatistics.csv  Bit,Set,Unset,Total and a line per bit.
 * The groups and the counts come from the device, the text is written on the host.  Host signatures. */
int em2_analyze_lsh_signatures(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, const char* directory);

/* ------------------------------------------------------------------------------------------------------
 * The gene graph: the consumer of the SimilarGenePairs-<name> objects.  csrc/em2_gene_graph.hip, DESIGN.md 3.14.
 * Integer / index work, nothing is computed from a similarity: every output is bit-exact.
 * ------------------------------------------------------------------------------------------------------ */

/* The GeneGraph constructor (src/GeneGraph.cpp:22-104), which ExpressionMatrix::createGeneGraph
 * (src/ExpressionMatrixGeneGraph.cpp:44-89) calls after its lookups, and GeneGraph::getConnectivity (src/GeneGraph.cpp:108-143):
 *   vertices   one per gene of the graph's gene set S, in set order (:40-43);
 *   edges      for every gene g0 of S in order that is also in the pairs' gene set P (:61-64), its stored list is walked up to
 *              the first entry with float similarity < double similarityThreshold (:71: equal stays, a NaN stays and the walk
 *              goes on); a partner outside S is skipped and does not count (:76-77); every other one is an add_edge and counts,
 *              and the walk ends when the count EQUALS maxConnectivity (:80-83: 0, and the negative Python int that size_t
 *              turned into 2^64 - 1, never match -- no limit).  The out-edge container is boost::setS (src/GeneGraph.hpp:33-38):
 *              an add_edge of an edge that exists adds nothing, STILL COUNTS, and the edge keeps the similarity of its first
 *              insertion.  The edges come out in the order they were created;
 *   removal    every vertex without an edge is removed (:88-99); a gene whose own list selected nothing stays where another
 *              gene selected it;
 *   connectivity   per local id of S the (local id in S of the neighbour, similarity) of every incident edge; nothing for a
 *              removed gene.  WITHIN A LIST THE NEIGHBOURS ASCEND BY LOCAL ID.  That is this library's definition: the reference
 *              iterates a std::set keyed on listS vertex descriptors, which are heap pointers, so its order is undefined.
 * pairs [pairsGeneCount][k] (local ids in P) and usedCount [pairsGeneCount]: the SimilarGenePairs object, host memory
 * (em2_dev_gene_graph_create: device memory).  pairsGeneSet / graphGeneSet: the global ids of P and S, host memory in both
 * entries, strictly ascending (EM2_ERROR_INVALID_ARGUMENT otherwise).  graphGeneCount 0 is an error, as the reference's empty gene
 * set is; pairsGeneCount 0 is a graph without vertices.
 * Outside the contract, EM2_ERROR_INVALID_ARGUMENT and no guess: a stored pair (any of the usedCount[g] first of a gene of P,
 * walked or not) whose partner is the gene itself or a local id >= pairsGeneCount -- findSimilarGenePairs0 writes neither --
 * and a usedCount above k.
 * The result is an object: em2_gene_graph_sizes (vertices that stay, edges, vertices removed: the three numbers of the
 * reference's message, :101-103), then em2_gene_graph_get into arrays of those sizes (any may be NULL):
 *   vertices[vertexCount]          the local ids in S of the genes that stay, ascending;
 *   edgeGene0 / edgeGene1 / edgeSimilarity[edgeCount]   local ids in S, in insertion order;
 *   connectivityOffsets[graphGeneCount + 1], connectivityGenes / connectivitySimilarities[2 * edgeCount].
 * Not built: the Graphviz output, the layout, the SVG and the colouring by meta data (src/GeneGraph.cpp:146-,
 * src/ExpressionMatrixGeneGraph.cpp:114-173). */
typedef struct em2_gene_graph em2_gene_graph;
int em2_gene_graph_create(const em2_pair* pairs, const uint32_t* usedCount, uint32_t pairsGeneCount, uint32_t k,
                          const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                          double similarityThreshold, uint64_t maxConnectivity, em2_gene_graph** graph);
int em2_dev_gene_graph_create(const em2_pair* d_pairs, const uint32_t* d_usedCount, uint32_t pairsGeneCount, uint32_t k,
                              const uint32_t* pairsGeneSet, const uint32_t* graphGeneSet, uint32_t graphGeneCount,
                              double similarityThreshold, uint64_t maxConnectivity, em2_gene_graph** graph);
int em2_gene_graph_sizes(const em2_gene_graph* graph, uint32_t* vertexCount, uint64_t* edgeCount, uint32_t* removedCount);
int em2_gene_graph_get(const em2_gene_graph* graph, uint32_t* vertices, uint32_t* edgeGene0, uint32_t* edgeGene1, float* edgeSimilarity,
                       uint64_t* connectivityOffsets, uint32_t* connectivityGenes, float* connectivitySimilarities);
void em2_gene_graph_free(em2_gene_graph* graph);

/* ------------------------------------------------------------------------------------------------------
 * The layout of a graph in the plane.  csrc/em2_layout.hip, DESIGN.md 3.19.
 * The reference writes Graph.dot and runs Graphviz's sfdp (src/CellGraph.cpp:210-264).  This is the model sfdp minimises --
 * Hu's spring-electrical model -- at a single level with the exact N-body repulsion: no multilevel coarsening, no
 * approximation of the far field (both are options further down), no overlap removal, no edge smoothing.  The positions are not sfdp's; they are a function
 * of the input alone, bit for bit (every rounding and the shape of every sum are fixed).
 * ------------------------------------------------------------------------------------------------------ */

/* The graph: vertexCount vertices, edgeCount undirected, unweighted edges (edgeVertex0[e], edgeVertex1[e]).  A self-loop
 * contributes nothing, a repeated edge attracts twice.  With d = |p_i - p_j|, natural length K = 1 and C = 0.2 the force on
 * vertex i is
 *     sum over every j of (p_i - p_j) * C K^2 / max(d^2, 1e-30)  -  sum over the neighbours j of (p_i - p_j) * d / K  -  gravity * p_i
 * The start positions are a hash of (seed, vertex index), uniform on a square of side sqrt(vertexCount) * K about the origin
 * (those of a vertex differ between two vertex counts by that factor only).  An iteration moves every vertex by
 * step * f / |f| (not at all where |f| = 0) and then adapts the step from the energy, the sum of |f|^2 in double: times 0.9
 * when it did not fall, divided by 0.9 after five falls in a row.  The run ends after maxIterationCount iterations or as soon as
 * step < tolerance * K; with maxIterationCount 0 the start positions come back.
 * The defaults (DESIGN.md 3.19 says on which graphs they were chosen; nothing is promised about the picture they give): */
#define EM2_LAYOUT_DEFAULT_SEED 231u
#define EM2_LAYOUT_DEFAULT_MAX_ITERATION_COUNT 300u
#define EM2_LAYOUT_DEFAULT_TOLERANCE 0.01
#define EM2_LAYOUT_DEFAULT_GRAVITY 0.02
#define EM2_LAYOUT_DEFAULT_INITIAL_STEP 1.0
typedef struct em2_layout_parameters {
    uint32_t seed;
    uint32_t maxIterationCount;
    double tolerance;   /* >= 0 */
    double gravity;     /* >= 0; 0 is allowed: nothing then holds the components of a disconnected graph together */
    double initialStep; /* >= 0, in units of K */
} em2_layout_parameters;
#define EM2_LAYOUT_PARAMETERS_DEFAULT                                                                                          \
    {EM2_LAYOUT_DEFAULT_SEED, EM2_LAYOUT_DEFAULT_MAX_ITERATION_COUNT, EM2_LAYOUT_DEFAULT_TOLERANCE, EM2_LAYOUT_DEFAULT_GRAVITY, \
     EM2_LAYOUT_DEFAULT_INITIAL_STEP}

/* iterationCount: the iterations done; step: the step after the last update; energy: the sum of |f|^2 of the last evaluation
 * (the positions before the last move), +infinity where there was no iteration. */
typedef struct em2_layout_result {
    uint32_t iterationCount;
    uint32_t reserved;
    double step;
    double energy;
} em2_layout_result;

/* x / y [vertexCount] receive the positions; result may be NULL.  em2_graph_layout: host pointers; em2_dev_graph_layout:
 * edgeVertex0 / edgeVertex1 / x / y in device memory (it takes its scratch from the library's cache and returns when the
 * positions are written).  vertexCount 0 is EM2_OK and writes nothing.  EM2_ERROR_INVALID_ARGUMENT: a null pointer (the edge
 * arrays may be NULL where edgeCount is 0), an edge end >= vertexCount (checked on the device before anything indexes with
 * it), a negative or NaN tolerance, gravity or initialStep.  EM2_ERROR_UNSUPPORTED: vertexCount above 2^30.
 * Not tied to cells: any graph given as two index arrays can be laid out. */
int em2_graph_layout(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                     const em2_layout_parameters* parameters, float* x, float* y, em2_layout_result* result);
int em2_dev_graph_layout(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                         const em2_layout_parameters* parameters, float* d_x, float* d_y, em2_layout_result* result);

/* For tests: one evaluation of f at the given positions x / y [vertexCount], no move.  fx / fy [vertexCount] and *energy (may
 * be NULL) receive the forces and the sum of |f|^2.  Host pointers; the same checks. */
int em2_graph_layout_forces(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                            double gravity, const float* x, const float* y, float* fx, float* fy, double* energy);

/* The same model with the repulsion approximated beyond a vertex's neighbourhood: a pyramid of fixed depth over the bounding
 * square of the current positions.  An option next to the exact entries above, which stay as they are.  Still
 * a function of the input alone, bit for bit: every sum that many threads share is an integer sum.  Per force evaluation, at
 * the current float32 positions:
 *   box      xmin, xmax, ymin, ymax over all vertices; S = fmaxf(xmax - xmin, ymax - ymin).  S == 0: every vertex is in cell 0
 *            of every level.
 *   q        u = fminf(fmaxf((x - xmin) / S, 0), 1), q = uint32_t(u * 2^31) <= 2^31, per axis.  Nothing but q forms an index.
 *   levels   level l = 0 ... D has 2^l x 2^l cells; the cell of a vertex is min(2^l - 1, q >> (31 - l)) per axis.  D is the
 *            smallest value in 0 ... EM2_LAYOUT_MAX_DEPTH with EM2_LAYOUT_LEAF_TARGET * 4^D >= vertexCount, else the maximum;
 *            `depth` forces it (EM2_LAYOUT_DEPTH_AUTO: that rule).
 *   order    the vertices sorted by (morton(cell at level D), vertex), one radix sort of distinct keys: within a leaf they
 *            ascend by index.
 *   moments  per cell a count and the integer sums of q_x and q_y (uint64); a parent is the sum of its four children.  The
 *            centroid of a non-empty cell, one rounding from double: m = float(double(xmin) + double(S) * t) with
 *            t = double(sum q) / (double(count) * 2^31).
 *   far      for l = 2 ... D ascending, (ax, ay) the vertex's cell: the cells (bx, by) of level l with by ascending from
 *            2 ((ay >> 1) - 1) to 2 ((ay >> 1) + 1) + 1 and bx likewise inside, that are inside the grid, not empty and not
 *            within Chebyshev distance 1 of (ax, ay) -- at most 27 a level.  Per cell dx = x_i - m_x, dy = y_i - m_y,
 *            d2 = fmaf(dx, dx, dy * dy), w = (0.2f * float(count)) / fmaxf(d2, 1e-30f), fx = fmaf(dx, w, fx), fy likewise:
 *            one sequential sum from +0.
 *   near     the leaves within Chebyshev distance 1 of the vertex's own (by ascending, then bx), their vertices in ascending
 *            index, the exact pair term: a second sequential sum from +0.  The repulsion is far + near.
 * Everything else (attraction, gravity, the move, the energy in vertex order, the step, the start positions, the stop rule)
 * is that of the exact entries.  Known limits: the cells are separated by one cell width only (theta <= 1 in Barnes-Hut's
 * terms, where sfdp uses 0.6); a layout that collapses into a few dense clusters fills few leaves, and the near field then
 * grows towards the exact cost -- the tree is not adaptive.  No multilevel coarsening (em2_graph_layout_multilevel below).
 * The checks, codes and texts are those of the exact entries; a depth that is neither EM2_LAYOUT_DEPTH_AUTO nor
 * <= EM2_LAYOUT_MAX_DEPTH is EM2_ERROR_INVALID_ARGUMENT. */
#define EM2_LAYOUT_DEPTH_AUTO 0xffffffffu
#define EM2_LAYOUT_MAX_DEPTH 10u
#define EM2_LAYOUT_LEAF_TARGET 8u /* part of the contract: it decides the automatic depth and so the bits of the result */
int em2_graph_layout_pyramid(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                             const em2_layout_parameters* parameters, uint32_t depth, float* x, float* y, em2_layout_result* result);
int em2_dev_graph_layout_pyramid(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                                 const em2_layout_parameters* parameters, uint32_t depth, float* d_x, float* d_y,
                                 em2_layout_result* result);
int em2_graph_layout_forces_pyramid(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                                    double gravity, uint32_t depth, const float* x, const float* y, float* fx, float* fy,
                                    double* energy);

/* The same model over a hierarchy of graphs, as sfdp does it: coarsen by matching, lay the coarsest graph out, then refine
 * level by level.  An option next to the entries above, which stay as they are, bit for bit.  Still a
 * function of the input alone: everything about the levels is integer arithmetic, and the forces keep their fixed shapes.
 *   levels     level 0 is the input graph.  Level l has n_l vertices, each with an integer mass, and merged edges (a, b),
 *              a < b, each pair once, with an integer weight.  At level 0 every mass is 1 and the weight of (a, b) is the
 *              number of input edges between a and b; self-loops carry no weight and take no part in coarsening.
 *   hash       mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *              z ^ z >> 31 (uint64: the start positions' hash is mix(seed << 32 | vertex)).  h(seed, level, w) =
 *              mix(mix(seed << 32 | level) ^ w) for a 64-bit w.
 *   matching   the greedy maximal matching over the level's merged edges in descending order of the total key (weight,
 *              h(seed, level, a << 32 | b), a, b).  The device finds it in rounds of locally dominant edges: every unmatched
 *              vertex points at the other end of its best live edge (one to an unmatched neighbour), two vertices that point at
 *              each other are matched, until no live edge is left (one counter comes back to the host per round).  Under a
 *              total order that is the greedy matching, not merely a maximal one.
 *   groups     an unmatched vertex or a matched pair; its representative is its smaller index; the coarse ids ascend with
 *              the representative; the coarse mass is the sum of the group's masses; the coarse edges are the fine edges with
 *              mapped ends, those inside a group dropped, parallel ones merged and their weights added.
 *   stop       level l is the coarsest when n_l <= EM2_LAYOUT_COARSEST, or when the next level would have
 *              4 n_(l+1) > 3 n_l (that level is discarded), or when l + 1 == EM2_LAYOUT_MAX_LEVELS.  A graph that does not
 *              coarsen -- a star, a graph without edges, any graph of at most 32 vertices -- has one level.
 *   force      at a level l >= 1 the force on i is that of a group of m_i coincident level-0 vertices, divided by m_i:
 *                  sum over every j of m_j (p_i - p_j) C / max(d^2, 1e-30)
 *                    - (1 / m_i) sum over the edges (i, j), j ascending, of w_ij (p_i - p_j) d  -  gravity * p_i
 *              with these roundings: the repulsion weight is (0.2f * float(m_j)) / fmaxf(d2, 1e-30f); an attraction term is
 *              ax = fmaf(dx, d * float(w_ij), ax); the attraction sums are divided by float(m_i) once, then subtracted.  The
 *              sum shapes, the energy, the move and the step control are those of the single-level entries; with all masses
 *              and weights 1 so are the bits.  In the pyramid a cell's count is its mass sum (float(count) is the far
 *              weight's factor as before), its moments are the sums of m * q (at most 2^61), a near pair carries float(m_j),
 *              and the automatic depth is that of n_l.
 *   level 0    is the input as the single-level entries see it, through their unweighted kernels: a repeated edge attracts
 *              twice (two terms, not one of weight 2).
 *   schedule   the coarsest level starts from the hash of (seed, vertex) on the square of side sqrtf(float(vertexCount)) --
 *              the INPUT's vertex count -- and runs the adaptive iteration with the caller's parameters.  Then level by level
 *              down to 0: a representative takes its group's position, the other member of a pair that position plus
 *              (ux, uy), the two 24-bit halves of h(seed, l, vertex) as the start positions form them, in [-0.5, 0.5)^2 (l: the
 *              level that receives the positions; coincident vertices would never separate, their pair terms being exact
 *              zeros).  Each level starts again at initialStep with an energy of +infinity and has the whole iteration budget.
 *              A graph of one level gets exactly what the single-level entry of the same `depth` returns.
 *   depth      EM2_LAYOUT_DEPTH_EXACT: every level uses the exact repulsion.  EM2_LAYOUT_DEPTH_AUTO: level 0 is
 *              em2_graph_layout_pyramid's level at the automatic depth; a coarse level of at most EM2_LAYOUT_EXACT_LIMIT
 *              vertices is exact, a larger one uses the pyramid at the automatic depth of n_l.  0 ... EM2_LAYOUT_MAX_DEPTH:
 *              every level uses the pyramid at that depth (for tests).
 * Known limits: a lane scans the whole adjacency of its vertex in a matching round, so a hub of 10^6 neighbours serialises the
 * round; isolated vertices never merge, so a graph that is mostly isolated vertices stops coarsening early; still no overlap
 * removal and no edge smoothing.  All levels stay in device memory (their sizes sum to at most four times the finest).
 * The checks, codes and texts are those of the entries above; edgeCount >= 2^32 is EM2_ERROR_UNSUPPORTED (the weights are
 * uint32).  An error return leaves x, y, result and levels as they were. */
#define EM2_LAYOUT_DEPTH_EXACT 0xfffffffeu
#define EM2_LAYOUT_COARSEST 32u
#define EM2_LAYOUT_MAX_LEVELS 32u
#define EM2_LAYOUT_EXACT_LIMIT 4096u
/* What a multilevel run did, level 0 first.  edgeCount: the merged edges; matchingRounds: the rounds of the matching that made
 * the level from the one below it (0 at level 0); iterationCount: the iterations at the level.  The entries past levelCount
 * are 0.  (em2_layout_result: iterationCount is the total over the levels, step and energy are those of level 0's end.) */
typedef struct em2_layout_levels {
    uint32_t levelCount;
    uint32_t reserved;
    uint32_t vertexCount[EM2_LAYOUT_MAX_LEVELS];
    uint32_t matchingRounds[EM2_LAYOUT_MAX_LEVELS];
    uint32_t iterationCount[EM2_LAYOUT_MAX_LEVELS];
    uint32_t reserved2[EM2_LAYOUT_MAX_LEVELS];
    uint64_t edgeCount[EM2_LAYOUT_MAX_LEVELS];
} em2_layout_levels;
int em2_graph_layout_multilevel(uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1, uint64_t edgeCount,
                                const em2_layout_parameters* parameters, uint32_t depth, float* x, float* y, em2_layout_result* result,
                                em2_layout_levels* levels);
int em2_dev_graph_layout_multilevel(uint32_t vertexCount, const uint32_t* d_edgeVertex0, const uint32_t* d_edgeVertex1, uint64_t edgeCount,
                                    const em2_layout_parameters* parameters, uint32_t depth, float* d_x, float* d_y,
                                    em2_layout_result* result, em2_layout_levels* levels);

/* For tests: one coarsening step.  The graph: vertexCount > 0 vertices with masses (mass NULL: 1; else each >= 1 and their sum at
 * most 2^30) and any edges with weights (edgeWeight NULL: 1; their sum below 2^32), merged first as level 0 is: loops dropped,
 * repeats added.  `level` enters the hash.  mate [vertexCount] (0xffffffff where unmatched), coarseOf [vertexCount];
 * coarseMass [vertexCount] and coarseEdge0 / coarseEdge1 / coarseWeight [edgeCount] are filled from the front (ascending by
 * (coarseEdge0, coarseEdge1)); *coarseVertexCount, *matchingRounds, *coarseEdgeCount.  Host pointers, none NULL but mass and
 * edgeWeight (the edge arrays where edgeCount is 0).  The stop rule is not applied. */
int em2_graph_layout_coarsen(uint32_t vertexCount, const uint32_t* mass, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                             const uint32_t* edgeWeight, uint64_t edgeCount, uint32_t seed, uint32_t level, uint32_t* mate,
                             uint32_t* coarseOf, uint32_t* coarseVertexCount, uint32_t* matchingRounds, uint32_t* coarseMass,
                             uint32_t* coarseEdge0, uint32_t* coarseEdge1, uint32_t* coarseWeight, uint64_t* coarseEdgeCount);

/* For tests: em2_graph_layout_forces through the weighted kernels, with masses and weighted edges as above (taken as they
 * are, not merged: two edges between the same vertices are two terms, in the order given).  depth: EM2_LAYOUT_DEPTH_EXACT,
 * EM2_LAYOUT_DEPTH_AUTO or 0 ... EM2_LAYOUT_MAX_DEPTH. */
int em2_graph_layout_forces_weighted(uint32_t vertexCount, const uint32_t* mass, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                                     const uint32_t* edgeWeight, uint64_t edgeCount, double gravity, uint32_t depth, const float* x,
                                     const float* y, float* fx, float* fy, double* energy);

/* ------------------------------------------------------------------------------------------------------
 * The contingency table of two labelings of n items.  csrc/em2_contingency.hip, DESIGN.md 3.16.  Integers only: every output
 * is exact.
 * ------------------------------------------------------------------------------------------------------ */

/* What ExpressionMatrix::computeMetaDataRandIndex (src/ExpressionMatrix.cpp:1369-1381) fills with four string copies and two
 * std::map look-ups per cell, and what computeRandIndex (src/randIndex.hpp:38-85) sums over it: the table whose cell (i, j)
 * counts the items with id0 == i and id1 == j.  id0[n] with id0[i] < n0, id1[n] with id1[i] < n1, host memory
 * (em2_dev_contingency: device memory).  An id out of range is EM2_ERROR_INVALID_ARGUMENT: the kernels test an id before they
 * form an address with it and write nothing for that element.  n0 and n1 positive; n below 2^32 (EM2_ERROR_UNSUPPORTED).
 * path: 0 chooses -- a private table per workgroup in LDS where n0 * n1 <= 16384, else a radix sort of the (id0, id1) keys --
 * 1 and 2 force the LDS path (n0 * n1 > 16384: EM2_ERROR_INVALID_ARGUMENT) and the sort path.  Both give the same result.
 * The table is returned sparse, because a field with many values (createMetaDataFromClusterGraph gives every unclustered cell a
 * value of its own) makes the reference's dense n0 x n1 vector<vector<size_t>> impossible to allocate.  The result is an
 * object: em2_contingency_sizes (n0, n1, n, the cells that are not zero, the path that ran: 1 or 2; any may be NULL), then
 * em2_contingency_get into arrays of those sizes (any may be NULL):
 *   rowTotals[n0], columnTotals[n1]           the items with id0 == i, with id1 == j;
 *   i0 / i1 / count[nonZeroCount]             the cells that are not zero, ascending by (i0, i1);
 *   sums[3]                                   sum of v (v - 1) over the cells, of t (t - 1) over the row totals, over the column
 *                                             totals: 2 a, 2 (a + b) and 2 (a + c) of src/randIndex.hpp:63-85.
 * (The host-pointer entry is em2_contingency_create because C has one name space for the type and the functions.) */
typedef struct em2_contingency em2_contingency;
int em2_contingency_create(const uint32_t* id0, const uint32_t* id1, uint64_t n, uint32_t n0, uint32_t n1, int path, em2_contingency** table);
int em2_dev_contingency(const uint32_t* d_id0, const uint32_t* d_id1, uint64_t n, uint32_t n0, uint32_t n1, int path, em2_contingency** table);
int em2_contingency_sizes(const em2_contingency* table, uint32_t* n0, uint32_t* n1, uint64_t* n, uint64_t* nonZeroCount, int* path);
int em2_contingency_get(const em2_contingency* table, uint64_t* rowTotals, uint64_t* columnTotals, uint32_t* i0, uint32_t* i1,
                        uint64_t* count, uint64_t* sums);
void em2_contingency_free(em2_contingency* table);

/* computeRandIndex (src/randIndex.hpp:58-97) from the three sums of em2_contingency_get and n, on the host, expression by
 * expression (the library is built without FMA contraction).  While n (n - 1) < 2^53 -- n <= 94906266 -- a, b, c, d, nBinomial2
 * and every partial sum of the reference's loops are integers a double holds, so the reference's sums are exact in any order and
 * the two results are the reference's bit for bit (NaN where it divides 0 by 0: n == 1, one value in both fields).  Above that
 * EM2_ERROR_UNSUPPORTED; n == 0 is the reference's CZI_ASSERT(rowCount > 0), EM2_ERROR_RUNTIME. */
int em2_rand_index(uint64_t sumCells, uint64_t sumRows, uint64_t sumColumns, uint64_t n, double* randIndex, double* adjustedRandIndex);

/* ------------------------------------------------------------------------------------------------------
 * Two cell graphs compared, and the colours of a cell graph's vertex groups.  csrc/em2_graph_compare.hip, DESIGN.md 3.24.
 * Integer sums and minima and single float operations: every output is the reference's, bit for bit.
 * ------------------------------------------------------------------------------------------------------ */

/* ExpressionMatrix::compareCellGraphs (src/ExpressionMatrixHttpServerGraphs.cpp:104-345) without its page.  Per graph g:
 * vertexCellIds_g[vertexCount_g] in host memory, as for em2_cell_graph_label_propagation, and the edges as vertex indices with
 * their similarities, edgeVertex0_g / edgeVertex1_g / edgeSimilarity_g[edgeCount_g] -- host memory here, DEVICE memory in
 * em2_dev_cell_graph_compare (what em2_dev_cell_graph_edges left there), so a device-resident chain never brings its edges to
 * the host.  Fewer than 2^32 edges per graph (EM2_ERROR_UNSUPPORTED).
 *   - An edge is keyed by the cell ids of its two ends, the smaller first (:156-179): the two graphs number their vertices
 *     independently.  Where a graph holds the same unordered cell pair more than once, in either orientation, the first in edge
 *     order counts (map::insert does not overwrite, :166 and :178).  edgeCount0 / edgeCount1 of the result are the sizes of
 *     those two maps (:301-302), not the input counts.
 *   - commonVertexCount is the size of std::set_intersection of the two sorted id lists (:146-149), a multiset intersection:
 *     an id that one list holds a times and the other b times counts min(a, b).
 *   - commonEdgeCount: the keys both maps hold (:191-194).  commonIdenticalEdgeCount: those with similarity0 == similarity1
 *     as floats (:197-199); +0 and -0 are identical.
 *   - The bin of a common edge is 0.01f * std::round((similarity1 - similarity0) / 0.01f) (:200-201), every operation a
 *     correctly rounded float operation and the rounding to the nearest integer with ties away from zero.  The bins are keyed by
 *     the value of that product, as in the reference's std::map<float, size_t> (:189, :202-207); it can be +-inf.  The two zeros
 *     are one bin, and binDelta gives it the sign of the key that map keeps: the one inserted first, which is the product of
 *     the first common edge, ascending by (cellA, cellB), that falls into the bin.
 *   - A common edge whose difference is not a number (a NaN similarity, or two infinities of one sign) makes that map
 *     ill-formed: EM2_ERROR_UNSUPPORTED, and the message names the two cells.  A NaN on an edge only one graph has is ignored,
 *     as in the reference.
 *   - An edge whose two ends are the same cell is the reference's CZI_ASSERT(cellIdA != cellIdB) (:161, :173):
 *     EM2_ERROR_RUNTIME.  A vertex index that is not below vertexCount_g is EM2_ERROR_INVALID_ARGUMENT: the kernel tests it
 *     before it forms an address with it.  Neither creates an object.  Graph 0 is examined first, and in a graph the index
 *     error is reported before the other.
 * path: 0 counts the bins with |round(...)| <= 2048 in a table per workgroup in LDS and sends the other products through a
 * sorted list; 1 sends every product through the list (tests: both give the same result).
 * The result is an object: em2_graph_comparison_sizes (any pointer may be NULL; *path: the path that ran, as given), then
 * em2_graph_comparison_get into binDelta[binCount] / binCountOut[binCount], ascending by binDelta (either may be NULL). */
typedef struct em2_graph_comparison em2_graph_comparison;
int em2_cell_graph_compare(const uint32_t* vertexCellIds0, uint32_t vertexCount0, const uint32_t* edgeVertex0_0, const uint32_t* edgeVertex1_0,
                           const float* edgeSimilarity0, uint64_t edgeCount0, const uint32_t* vertexCellIds1, uint32_t vertexCount1,
                           const uint32_t* edgeVertex0_1, const uint32_t* edgeVertex1_1, const float* edgeSimilarity1, uint64_t edgeCount1,
                           int path, em2_graph_comparison** comparison);
int em2_dev_cell_graph_compare(const uint32_t* vertexCellIds0, uint32_t vertexCount0, const uint32_t* d_edgeVertex0_0,
                               const uint32_t* d_edgeVertex1_0, const float* d_edgeSimilarity0, uint64_t edgeCount0,
                               const uint32_t* vertexCellIds1, uint32_t vertexCount1, const uint32_t* d_edgeVertex0_1,
                               const uint32_t* d_edgeVertex1_1, const float* d_edgeSimilarity1, uint64_t edgeCount1, int path,
                               em2_graph_comparison** comparison);
int em2_graph_comparison_sizes(const em2_graph_comparison* comparison, uint64_t* commonVertexCount, uint64_t* edgeCount0,
                               uint64_t* edgeCount1, uint64_t* commonEdgeCount, uint64_t* commonIdenticalEdgeCount, uint64_t* binCount,
                               int* path);
int em2_graph_comparison_get(const em2_graph_comparison* comparison, float* binDelta, uint64_t* binCountOut);
void em2_graph_comparison_free(em2_graph_comparison* comparison);

/* CellGraph::assignColorsToGroups (src/CellGraph.cpp:794-862; the page's reuseColors, src/ExpressionMatrixHttpServerGraphs.cpp:
 * 900-913): colours for the groups of a graph's vertices such that no two groups joined by an edge share one, so that a few
 * colours serve many groups.  vertexGroup[vertexCount] in host memory; the edges as vertex indices, host memory here and DEVICE
 * memory in em2_dev_graph_group_colors.  Fewer than 2^32 edges (EM2_ERROR_UNSUPPORTED); a vertex index that is not below
 * vertexCount is EM2_ERROR_INVALID_ARGUMENT (tested on the device before an address is formed with it).
 *   groupCount                      the largest group + 1 (:799-808), 0 without vertices: a group no vertex has gets a colour too;
 *   pairGroup0 < pairGroup1 [pairCount], ascending: the group graph (:813-825), with pairEdgeCount, the edges of the graph between
 *                                   the two groups.  They are the cells off the diagonal of the contingency table of
 *                                   (group of vertex 0, group of vertex 1) over the edges (em2_dev_contingency), folded over it;
 *   colorTable[groupCount]          the reference's greedy (:830-861), on the host: the groups ascending, each the first index c
 *                                   at which the sorted distinct colours of its adjacent smaller groups differ from c, else their
 *                                   number.
 * path is handed to em2_dev_contingency (0, 1 = LDS: groupCount^2 <= 16384, 2 = sort); *path of em2_group_colors_sizes is the
 * one that ran, 0 where there was no edge.  em2_group_colors_get: any pointer may be NULL. */
typedef struct em2_group_colors em2_group_colors;
int em2_graph_group_colors(const uint32_t* vertexGroup, uint32_t vertexCount, const uint32_t* edgeVertex0, const uint32_t* edgeVertex1,
                           uint64_t edgeCount, int path, em2_group_colors** colors);
int em2_dev_graph_group_colors(const uint32_t* vertexGroup, uint32_t vertexCount, const uint32_t* d_edgeVertex0,
                               const uint32_t* d_edgeVertex1, uint64_t edgeCount, int path, em2_group_colors** colors);
int em2_group_colors_sizes(const em2_group_colors* colors, uint32_t* groupCount, uint64_t* pairCount, int* path);
int em2_group_colors_get(const em2_group_colors* colors, uint32_t* pairGroup0, uint32_t* pairGroup1, uint64_t* pairEdgeCount,
                         uint32_t* colorTable);
void em2_group_colors_free(em2_group_colors* colors);

/* ------------------------------------------------------------------------------------------------------
 * ExpressionMatrix-level entry points: the methods the reference binds to Python (src/PythonModule.cpp),
 * operating by NAME on a data directory in the reference's memory-mapped formats.  Results are files in
 * that directory (SimilarPairs-<name>-{Info,Pairs,CellInfo}, Lsh-<name>-{Info,Signatures}), byte-compatible
 * with what the reference writes.  Errors the reference reports with std::runtime_error come back as
 * EM2_ERROR_RUNTIME with the reference's message text.
 * ------------------------------------------------------------------------------------------------------ */
typedef struct em2_matrix em2_matrix;

/* ExpressionMatrix(directoryName, allowReadOnly) for an existing directory (src/ExpressionMatrix.cpp:109-160);
 * opens only what the entries here read: CellExpressionCounts.{toc,data}, CellSet-*, GeneSet-*-{GlobalIds,LocalIds} and, where
 * the directory has them, the CellMetaData* files (read into host memory; see the cell meta data entries). */
int em2_matrix_open(const char* directoryName, em2_matrix** matrix);
void em2_matrix_close(em2_matrix* matrix);

/* ExpressionMatrix::findSimilarPairs4 (src/ExpressionMatrixLsh.cpp:155-303; bound at src/PythonModule.cpp:802-824,
 * defaults AllGenes, AllCells, k=100, similarityThreshold=0.2, lshCount=1024, seed=231). */
int em2_matrix_find_similar_pairs4(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* similarPairsName, size_t k, double similarityThreshold,
                                   size_t lshCount, unsigned int seed);

/* ExpressionMatrix::computeLshSignatures (src/ExpressionMatrixLsh.cpp:1150-1192; src/PythonModule.cpp:945-953). */
int em2_matrix_compute_lsh_signatures(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                      const char* lshName, size_t lshCount, unsigned int seed);

/* ExpressionMatrix::analyzeLsh(geneSetName, cellSetName, lshCount, seed, csvDownsample) (src/ExpressionMatrixLsh.cpp:
 * 1244-1367, bound without defaults at src/PythonModule.cpp:940-944): subset + signatures + em2_analyze_lsh.  The
 * reference writes "Lsh-analysis.csv" and "LSH-analysis-statistics.csv" into the working directory; outputDirectory
 * (NULL or "": the working directory) says where. */
int em2_matrix_analyze_lsh(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, size_t lshCount,
                           unsigned int seed, double csvDownsample, const char* outputDirectory);

/* ExpressionMatrix::createSignatureGraph's lookups (src/ExpressionMatrixSignatureGraph.cpp:50-67; bound at
 * src/PythonModule.cpp:984-1004) and em2_signature_graph_create on the signatures of Lsh-<lshName>: "Cell set X does not
 * exist." / "... is empty.", "LSH object L has a number of cells inconsistent with cell set C.".  The cells of the graph are
 * ids local to the cell set (em2_matrix_cell_set gives the global ones).  The names of the graphs ("Signature graph X already
 * exists." / "... does not exists.") are kept by the caller: the reference keeps its graphs in memory only. */
int em2_matrix_create_signature_graph(em2_matrix* matrix, const char* cellSetName, const char* lshName, uint64_t minCellCount,
                                      em2_signature_graph** graph);

/* ExpressionMatrix::analyzeLshSignatures (src/ExpressionMatrixLsh.cpp:1372-1474; bound at src/PythonModule.cpp:954-962 with
 * the defaults AllGenes, AllCells, 1024, 231): the subset, its signatures (the projection of em2_matrix_compute_lsh_signatures;
 * no tmp-Lsh files are created), then em2_analyze_lsh_signatures into outputDirectory (NULL or "": the working directory). */
int em2_matrix_analyze_lsh_signatures(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, size_t lshCount,
                                      unsigned int seed, const char* outputDirectory);

/* ExpressionMatrix::createGeneGraph's lookups (src/ExpressionMatrixGeneGraph.cpp:65-77; bound at src/PythonModule.cpp:1137-1161)
 * and em2_gene_graph_create on SimilarGenePairs-<similarGenePairsName>: "Gene set X does not exist." / "Gene set X is empty.",
 * then the errors of em2_similar_gene_pairs_read for a missing or inconsistent object.  k is the reference's int: it becomes
 * maxConnectivity as (size_t) k, so 0 and every negative value mean no limit.  The ids of the graph are local to the gene set
 * (em2_matrix_gene_set gives the global ones).  The names of the graphs are kept by the caller, the reference's slips with them:
 * the name is checked against the SIGNATURE graphs ("Signature graph X already exists.", :63) and a second gene graph under an
 * existing name is built and then dropped by map::insert (:88); "Gene graph X does not exists." */
int em2_matrix_create_gene_graph(em2_matrix* matrix, const char* geneSetName, const char* similarGenePairsName, int64_t k,
                                 double similarityThreshold, em2_gene_graph** graph);

/* ExpressionMatrix::createGeneSetIntersection / createGeneSetUnion (src/ExpressionMatrixGeneSets.cpp:183-250) and
 * createGeneSetDifference (:254-305), on the host.  inputSetsNames: names separated by commas, split as boost::split does (an
 * empty piece is a name; nothing is trimmed); the result is std::set_intersection / std::set_union folded from the left, for the
 * difference std::set_difference of set 0 and set 1.  The reference does not throw here: it prints a line and returns false.
 * *created = 0 and EM2_OK then, and em2_last_error() is that line: "Gene set X already exists." for the output, then for the
 * first missing input "gene set X does not exists." (intersection, union; sic) / "Gene set X does not exists." (difference).
 * An empty result is a gene set without genes. */
int em2_matrix_create_gene_set_intersection(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName, int* created);
int em2_matrix_create_gene_set_union(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName, int* created);
int em2_matrix_create_gene_set_difference(em2_matrix* matrix, const char* inputSetName0, const char* inputSetName1,
                                          const char* outputSetName, int* created);

/* ExpressionMatrix::findSimilarPairs5 (src/ExpressionMatrixLsh.cpp:312-501; src/PythonModule.cpp:852-865,
 * default bucketOverflow=1000). */
int em2_matrix_find_similar_pairs5(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, size_t lshSliceLength, size_t bucketOverflow);

/* ExpressionMatrix::findSimilarPairs6 (src/ExpressionMatrixLsh.cpp:842-1145; bound at src/PythonModule.cpp:866-880,
 * defaults k=100, similarityThreshold=0.2, permutedBitCount=64, seed=231). */
int em2_matrix_find_similar_pairs6(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, size_t permutationCount, size_t searchCount,
                                   size_t permutedBitCount, int seed);

/* ExpressionMatrix::findSimilarPairs7 (src/ExpressionMatrixLsh.cpp:507-703; bound at src/PythonModule.cpp:882-897). */
int em2_matrix_find_similar_pairs7(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, const int32_t* lshSliceLengths, uint32_t sliceLengthCount,
                                   uint32_t maxCheck, size_t log2BucketCount);


/* ExpressionMatrix::findSimilarPairs0 (src/ExpressionMatrixFindSimilarPairs.cpp:16-99; bound at
 * src/PythonModule.cpp:776-801, defaults k=100, similarityThreshold=0.2).  Unlike the LSH methods it leaves
 * lowestSimilarityIndex / lowestSimilarity in SimilarPairs-<name>-CellInfo.  Errors in the reference's order:
 * similarityThreshold > 1 (EM2_ERROR_RUNTIME), "Gene set X does not exist." / "is empty.", "Cell set X does not exist." /
 * "is empty.". */
int em2_matrix_find_similar_pairs0(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* similarPairsName, size_t k, double similarityThreshold);

/* ExpressionMatrix::analyzeSimilarPairs (src/ExpressionMatrixLsh.cpp:55-150; bound at src/PythonModule.cpp:921-925):
 * writes <similarPairsName>-analysis.csv and <similarPairsName>-analysis-statistics.csv into outputDirectory (NULL or
 * "": the working directory, as the reference). */
int em2_matrix_analyze_similar_pairs(em2_matrix* matrix, const char* similarPairsName, double csvDownsample,
                                     const char* outputDirectory);

/* ExpressionMatrix::computeCellSimilarity (src/ExpressionMatrix.cpp:1456-1537; bound at src/PythonModule.cpp:755-771):
 * the exact similarity of two cells given by GLOBAL id over the genes of a gene set.  Host code, one pair. */
int em2_matrix_compute_cell_similarity(em2_matrix* matrix, const char* geneSetName, uint32_t cellId0, uint32_t cellId1,
                                       double* similarity);

/* em2_cell_similarities_to_cell and em2_gene_expression_of_cells (above) for a gene set of the directory and GLOBAL cell ids:
 * out[i] is the similarity of cellId0 to cellIds[i], or gene globalGeneId's value in cellIds[i].  A cell id not below the cell
 * count: EM2_ERROR_INVALID_ARGUMENT.  "Gene set X is empty.", "Invalid normalization method." and the assertion for a gene outside
 * the gene set: EM2_ERROR_RUNTIME. */
int em2_matrix_cell_similarities_to_cell(em2_matrix* matrix, const char* geneSetName, uint32_t cellId0, const uint32_t* cellIds,
                                         uint32_t count, double* out);
int em2_matrix_gene_expression_of_cells(em2_matrix* matrix, const char* geneSetName, uint32_t globalGeneId, int normalizationMethod,
                                        const uint32_t* cellIds, uint32_t count, float* out);

/* colorByMetaDataInterpretedAsCategory for a graph over a cell set of the directory: see em2_pie_census_create above.  A global
 * cell id not below the cell count, or a vertex cell not below cellSetSize: EM2_ERROR_INVALID_ARGUMENT. */
int em2_matrix_pie_census(em2_matrix* matrix, uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                          const uint32_t* globalCellIds, uint32_t cellSetSize, const char* metaDataName, em2_pie_census** census);

/* ExpressionMatrix::compareSimilarPairs (src/ExpressionMatrixLsh.cpp:1199-1240): CompareSimilarPairs.csv in
 * outputDirectory (NULL or "": the working directory) with one line per cell whose stored count or last stored
 * similarity differ.  EM2_ERROR_RUNTIME where the two objects' gene sets or cell sets differ (CZI_ASSERT, :1208-1209).
 * Host code. */
int em2_matrix_compare_similar_pairs(em2_matrix* matrix, const char* similarPairsName0, const char* similarPairsName1,
                                     const char* outputDirectory);

/* ExpressionMatrix::removeSimilarPairs (src/ExpressionMatrixFindSimilarPairs.cpp:126-135). */
int em2_matrix_remove_similar_pairs(em2_matrix* matrix, const char* similarPairsName);

/* ExpressionMatrix::findSimilarGenePairs0 (src/ExpressionMatrixFindSimilarGenePairs.cpp:16-198; bound at
 * src/PythonModule.cpp:966-980, defaults AllGenes, AllCells, L2, k=100, similarityThreshold=0.2) without its csv: writes
 * SimilarGenePairs-<name>-{Info,Pairs,GeneInfo}.  Errors in the reference's order: "Gene set X does not exist." / "is empty.",
 * "Cell set X does not exist." / "is empty.". */
int em2_matrix_find_similar_gene_pairs0(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                        const char* similarGenePairsName, size_t k, double similarityThreshold);

/* ExpressionMatrix::removeSimilarGenePairs (src/ExpressionMatrixFindSimilarGenePairs.cpp:223-232). */
int em2_matrix_remove_similar_gene_pairs(em2_matrix* matrix, const char* similarGenePairsName);

/* ExpressionMatrix::computeGeneInformationContent (src/ExpressionMatrix.cpp:1947-1964; private in the reference, shown in
 * its HTTP page only) for the genes of a gene set over the cells of a cell set: out[size of the gene set].  The cells' norm
 * inverses come from the Cells file of the data directory (MemoryMapped::Vector<Cell>, src/Cell.hpp: seven doubles,
 * norm1Inverse at byte 24, norm2Inverse at byte 32, one record per global cell) where there is one, and are computed from the
 * cells' whole rows otherwise.  Errors: "Gene set X does not exist.", "Cell set X does not exist.". */
int em2_matrix_gene_information_content(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                        float* out);

/* em2_rank_genes for the genes of a gene set over the cells of a cell set, by name: the rows of the cells go to the device with
 * their global gene ids, the norm inverses are those of the cells' WHOLE rows (from the Cells file where there is one, as
 * em2_matrix_gene_information_content), the gene set is applied by the device subset, and the rest is em2_dev_rank_genes.
 * group[size of the cell set], in the order of the cell set: a group below groupCount, EM2_NO_GROUP, or EM2_GROUP_EXCLUDED --
 * such a cell is left out of the universe altogether (it is in no group and in no "rest"), which is how a caller ranks over a
 * part of a cell set without storing a new one.  The outputs as em2_rank_genes's, the genes in the gene set's local order;
 * zScore and auc may be NULL.  No cell left: every count is 0, zScore 0 and auc 0.5.
 * Errors: "Gene set X does not exist.", "Cell set X does not exist.". */
#define EM2_GROUP_EXCLUDED 0xfffffffeu
int em2_matrix_rank_genes(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                          const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2,
                          uint64_t* tieSum, double* zScore, double* auc);

/* ExpressionMatrix::createGeneSetUsingInformationContent (src/ExpressionMatrix.cpp:2022-2082; bound at
 * src/PythonModule.cpp:506-537): the genes of the existing set with double(information content) > threshold, in ascending
 * local id, as GeneSet-<newGeneSetName>-{GlobalIds,LocalIds}; usable by name at once.  Errors in the reference's order:
 * "Gene set X does not exist.", "Cell set X does not exist.", "Gene set X already exists.". */
int em2_matrix_create_gene_set_using_information_content(em2_matrix* matrix, const char* existingGeneSetName, const char* cellSetName,
                                                         int normalizationMethod, double geneInformationContentThreshold,
                                                         const char* newGeneSetName);

/* ExpressionMatrix::createWellExpressedGeneSet (src/ExpressionMatrixGeneSets.cpp:314-362; bound at
 * src/PythonModule.cpp:586-602): the genes of the input set with a stored entry in at least minCellCount cells of the cell
 * set.  "Gene set X already exists." is checked before the inputs are looked up (:322-329). */
int em2_matrix_create_well_expressed_gene_set(em2_matrix* matrix, const char* inputGeneSetName, const char* inputCellSetName,
                                              const char* outputGeneSetName, uint32_t minCellCount);

/* ExpressionMatrix::removeGeneSet (src/ExpressionMatrixGeneSets.cpp:12-32): "Gene set AllGenes cannot be removed.",
 * "Gene set X does not exist."; removes the two files. */
int em2_matrix_remove_gene_set(em2_matrix* matrix, const char* geneSetName);

/* Cell sets (host code).  A new set is the file CellSet-<name> (MemoryMapped::Vector<CellId>), known to this matrix under its
 * name at once and to every matrix opened on the directory afterwards.  Unlike the gene set operations these throw in the
 * reference, so every refusal is EM2_ERROR_RUNTIME with the reference's text.
 *   em2_matrix_create_cell_set     ExpressionMatrix::createCellSet (src/ExpressionMatrix.cpp:1626-1633) with
 *                                  CellSets::addCellSet (src/CellSets.cpp:65-83): "Cell set X already exists."; the ids are
 *                                  sorted and deduplicated.  DEPARTURE: an id not below the cell count is refused with
 *                                  EM2_ERROR_INVALID_ARGUMENT; the reference stores it and reads out of bounds later.
 *   ..._intersection / ..._union   createCellSetIntersectionOrUnion (:1642-1696): the output name first ("Cell set X already
 *                                  exists."), then the comma-separated input names, split at every comma (an empty piece is a
 *                                  name that does not exist): "Cell set X does not exist."; then std::set_intersection /
 *                                  std::set_union folded from left to right.
 *   ..._difference                 createCellSetDifference (:1700-1737): "Cell set X already exists.", then "Cell set X does
 *                                  not exists." (sic, :1715, :1720) for input 0, then input 1; std::set_difference.
 *   em2_matrix_downsample_cell_set downsampleCellSet (:1742-1777): "Cell set X does not exists." (sic, :1752); one draw of
 *                                  mt19937(seed) per input cell in set order, kept when draw * 2^-32 < probability
 *                                  (boost::uniform_01<> on boost::mt19937); the int seed wraps to 32 bits.  DEPARTURE: the
 *                                  reference does not look whether the output exists -- it maps a new file over the old one
 *                                  while its table keeps the old entry; here the call answers "Cell set X already exists."
 *                                  (after the input's check).
 *   em2_matrix_remove_cell_set     removeCellSet (src/ExpressionMatrixCells.cpp:113-116, src/CellSets.cpp:88-97): "Cell set X
 *                                  does not exist."; the file is removed.  DEPARTURE: the reference has no guard for AllCells
 *                                  and would leave a directory it cannot open again; here "Cell set AllCells cannot be
 *                                  removed." (ours, after removeGeneSet's for AllGenes).
 *   em2_matrix_cell_set_names      the names in std::map order (CellSets::cellSets, src/CellSets.hpp), each followed by a 0
 *                                  byte: pass names == NULL to get *bytes, then a buffer of that size. */
int em2_matrix_create_cell_set(em2_matrix* matrix, const char* cellSetName, const uint32_t* cellIds, uint32_t count);
int em2_matrix_create_cell_set_intersection(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName);
int em2_matrix_create_cell_set_union(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName);
int em2_matrix_create_cell_set_difference(em2_matrix* matrix, const char* inputSetName0, const char* inputSetName1,
                                          const char* outputSetName);
int em2_matrix_downsample_cell_set(em2_matrix* matrix, const char* inputCellSetName, const char* outputCellSetName, double probability,
                                   int seed);
int em2_matrix_remove_cell_set(em2_matrix* matrix, const char* cellSetName);
int em2_matrix_cell_set_names(em2_matrix* matrix, uint64_t* bytes, char* names);

/* Cell meta data: every cell carries (name, value) string pairs.  csrc/em2_meta_data.{h,cpp}, DESIGN.md 3.16.  The store is the
 * reference's files -- CellMetaData.{toc,data,freeSlots} (MemoryMapped::VectorOfLists<pair<StringId, StringId>>,
 * src/MemoryMappedVectorOfLists.hpp), CellMetaDataNames-* and CellMetaDataValues-* (MemoryMapped::StringTable<uint32_t>,
 * src/MemoryMappedStringTable.hpp), CellMetaDataNamesUsageCount (src/ExpressionMatrix.cpp:971-993) -- read by em2_matrix_open,
 * kept in host memory and written back by em2_matrix_flush and em2_matrix_close.  A directory without them is one where no
 * cell has a field; the first write creates the store with an empty list per cell and string tables of 1 << 12 slots that
 * double as the reference's do.  A store whose lists leave the node store or do not close is EM2_ERROR_IO.  A cell id not below
 * the cell count is EM2_ERROR_INVALID_ARGUMENT (the reference reads out of bounds).
 *   em2_matrix_set_cell_meta_data          ExpressionMatrix::setCellMetaData (src/ExpressionMatrix.cpp:942-967): the name and
 *                                          the value enter their tables, in that order; the value of the cell's first node of
 *                                          that name is replaced, else a node is appended and the name's usage count grows.
 *   em2_matrix_get_cell_meta_data_value    getCellMetaData(cellId, name) (:880-907): "" for an unknown name or a cell without
 *                                          it.  value == NULL: *bytes is set; else *bytes is the buffer's size on entry.
 *   em2_matrix_get_cell_meta_data          getCellMetaData(cellId) (:913-922): name, 0, value, 0, ... in list order; two calls
 *                                          as above.  (getCellsMetaData, :928-937, is a loop over this.)
 *   em2_matrix_remove_cell_meta_data       removeCellMetaData (:998-1029): "Cell set X not found."; an unknown name does
 *                                          nothing; else the first node of that name goes for every cell of the set, its slot
 *                                          becomes the next one to be reused, the usage count shrinks.
 *   em2_matrix_create_cell_set_using_meta_data   createCellSetUsingMetaData (:1560-1622): "Cell set X already exists." first;
 *                                          then the std::regex (default flags; an invalid one is EM2_ERROR_RUNTIME with
 *                                          std::regex_error's text and no set is made); then ALL cells, each judged by its first
 *                                          node of that name: std::regex_match of the whole value, or string equality.  The
 *                                          verdict is formed once per value, not per cell.  The set is stored as
 *                                          em2_matrix_create_cell_set stores one.
 *   em2_matrix_compute_meta_data_rand_index      computeMetaDataRandIndex (:1328-1390): "Cell set X not found.", "Meta data
 *                                          field X not found." for name 0, then name 1; an empty cell set is computeRandIndex's
 *                                          CZI_ASSERT(rowCount > 0) (EM2_ERROR_RUNTIME).  The host walks the lists of the set
 *                                          once and writes one compact id per cell and field (the distinct value ids of the
 *                                          field within the set, ascending; a cell without the field and a stored "" share one,
 *                                          as the reference hands both out as ""); the table is em2_contingency_create, the
 *                                          doubles em2_rand_index: above 94906266 cells EM2_ERROR_UNSUPPORTED.
 *   em2_matrix_meta_data_table             histogramMetaData (:1301-1323) of field 0 and, unless metaDataName1 is NULL, of
 *                                          field 1 -- count descending, then value ascending as std::string compares -- and the
 *                                          contingency table of :1369-1381 with rows and columns in that order, sparse.  The
 *                                          same checks.  em2_meta_data_table_sizes, then em2_meta_data_table_get (any may be
 *                                          NULL): values0[valueBytes0] (every value followed by a 0 byte), counts0[valueCount0],
 *                                          the same for field 1, row / column / count[nonZeroCount] ascending by (row, column),
 *                                          sums[4] = the three of em2_contingency_get and n.
 *                                          em2_meta_data_table_cell_rows: cellRow[size of the cell set], for every cell of the
 *                                          set in its order the place of its value of field 0 in values0 (the groups of
 *                                          rankGenesByMetaData). */
typedef struct em2_meta_data_table em2_meta_data_table;
int em2_matrix_set_cell_meta_data(em2_matrix* matrix, uint32_t cellId, const char* name, const char* value);
int em2_matrix_get_cell_meta_data_value(em2_matrix* matrix, uint32_t cellId, const char* metaDataName, uint64_t* bytes, char* value);
int em2_matrix_get_cell_meta_data(em2_matrix* matrix, uint32_t cellId, uint64_t* bytes, char* pairs);
int em2_matrix_remove_cell_meta_data(em2_matrix* matrix, const char* cellSetName, const char* metaDataName);
int em2_matrix_create_cell_set_using_meta_data(em2_matrix* matrix, const char* cellSetName, const char* metaDataFieldName,
                                               const char* matchString, int useRegex);
int em2_matrix_compute_meta_data_rand_index(em2_matrix* matrix, const char* cellSetName, const char* metaDataName0,
                                            const char* metaDataName1, double* randIndex, double* adjustedRandIndex);
int em2_matrix_meta_data_table(em2_matrix* matrix, const char* cellSetName, const char* metaDataName0, const char* metaDataName1,
                               em2_meta_data_table** table);
int em2_meta_data_table_sizes(const em2_meta_data_table* table, uint64_t* valueCount0, uint64_t* valueCount1, uint64_t* valueBytes0,
                              uint64_t* valueBytes1, uint64_t* nonZeroCount, int* path);
int em2_meta_data_table_get(const em2_meta_data_table* table, char* values0, uint64_t* counts0, char* values1, uint64_t* counts1,
                            uint64_t* row, uint64_t* column, uint64_t* count, uint64_t* sums);
int em2_meta_data_table_cell_rows(const em2_meta_data_table* table, uint32_t* cellRow);
void em2_meta_data_table_free(em2_meta_data_table* table);
/* Writes what the matrix holds in memory and has changed (the meta data store) to its files. */
int em2_matrix_flush(em2_matrix* matrix);

/* getDenseExpressionMatrix (src/PythonModule.cpp:78-154) for a gene set and a cell set of the directory: the rows
 * [rowBegin, rowEnd) of the cell set into out[(row - rowBegin) * geneSetSize + localGene] (see em2_dev_dense_expression for the
 * arithmetic and elementType).  Only those rows travel to the device, with the gene set applied there.  In the reference's
 * order: "Gene set X does not exist.", "Gene set X is empty.", "Cell set X does not exist.", "Cell set X is empty.", "Invalid
 * normalization method." (EM2_ERROR_RUNTIME); then rowBegin <= rowEnd <= the cell set's size and elementType
 * (EM2_ERROR_INVALID_ARGUMENT).  rowBegin == rowEnd makes the checks and writes nothing (out may be NULL). */
int em2_matrix_dense_expression(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                int elementType, uint32_t rowBegin, uint32_t rowEnd, void* out);

/* The stored (gene id, count) entries of a cell, ascending by global gene id -- what ExpressionMatrix::getCellExpressionCounts
 * (src/ExpressionMatrix.cpp:1030-1168 with its siblings) reads -- from the memory-mapped row: pass out == NULL to get *count,
 * then out[*count].  A cell id not below the cell count: EM2_ERROR_INVALID_ARGUMENT (the reference reads out of bounds). */
int em2_matrix_cell_expression_counts(em2_matrix* matrix, uint32_t cellId, uint64_t* count, em2_count* out);

/* ExpressionMatrixSubset (src/ExpressionMatrixSubset.cpp:9-42) as plain arrays, for drivers that shard the work
 * themselves: first call with toc == NULL to get the sizes, then with toc[cellCount+1] and data[nnz]. */
int em2_matrix_subset(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, uint32_t* geneCount,
                      uint32_t* cellCount, uint64_t* nnz, uint64_t* toc, em2_count* data);

/* SimilarPairs files: constructor + copy (src/SimilarPairs.cpp:11-42,369-379) from already selected and
 * sorted pairs; and the existing-object constructor (:47-83) with its hash / length checks.  For the read,
 * pass pairs/usedCount == NULL to get only k and cellCount. */
int em2_similar_pairs_write(const char* directoryName, const char* similarPairsName, const char* geneSetName,
                            const char* cellSetName, size_t k, uint32_t cellCount, const em2_pair* pairs,
                            const uint32_t* usedCount);
int em2_similar_pairs_read(const char* directoryName, const char* similarPairsName, uint64_t* k,
                           uint64_t* cellCount, em2_pair* pairs, uint32_t* usedCount);

/* SimilarPairs::Info (src/SimilarPairs.hpp:188-198): k, cell count and the names of the gene / cell set the object was
 * built on; name buffers must hold 256 bytes.  Same consistency checks as em2_similar_pairs_read. */
int em2_similar_pairs_info(const char* directoryName, const char* similarPairsName, uint64_t* k, uint64_t* cellCount,
                           char* geneSetName, char* cellSetName);

/* SimilarGenePairs files: the constructor for a new object (src/SimilarGenePairs.cpp:8-48) from already selected and sorted
 * pairs[geneCount][k] (local gene ids), and the existing-object constructor (:53-89) with its hash / length checks.
 * SimilarGenePairs::Info (src/SimilarGenePairs.hpp:138-153) is SimilarPairs::Info with the NormalizationMethod enum appended
 * (544 bytes, the enum at byte 536).  For the read every pointer after geneCount may be NULL; name buffers hold 256 bytes. */
int em2_similar_gene_pairs_write(const char* directoryName, const char* similarGenePairsName, const char* geneSetName,
                                 const char* cellSetName, size_t k, int normalizationMethod, uint32_t geneCount, const em2_pair* pairs,
                                 const uint32_t* usedCount);
int em2_similar_gene_pairs_read(const char* directoryName, const char* similarGenePairsName, uint64_t* k, uint64_t* geneCount,
                                int* normalizationMethod, char* geneSetName, char* cellSetName, uint64_t* geneSetHash,
                                uint64_t* cellSetHash, em2_pair* pairs, uint32_t* usedCount);

/* A cell set of the data directory (CellSet-<name>, src/CellSets.hpp:15): pass ids == NULL to get the count. */
int em2_matrix_cell_set(em2_matrix* matrix, const char* cellSetName, uint32_t* count, uint32_t* ids);

/* The global gene ids of a gene set of the data directory (GeneSet-<name>-GlobalIds, src/GeneSet.hpp), ascending: local gene
 * id i is globalIds[i].  Pass globalIds == NULL to get the count. */
int em2_matrix_gene_set(em2_matrix* matrix, const char* geneSetName, uint32_t* count, uint32_t* globalIds);

/* Lsh files Lsh-<name>-{Info,Signatures} (src/Lsh.hpp:136-141, src/Lsh.cpp:26-28,48-64,148). */
int em2_lsh_write(const char* directoryName, const char* lshName, uint64_t cellCount, uint64_t lshCount,
                  const uint64_t* signatures);
int em2_lsh_read(const char* directoryName, const char* lshName, uint64_t* cellCount, uint64_t* lshCount,
                 uint64_t* signatures);

/* Tooling for tests and benchmarks -- NOT a reference API.  Creates a directory that holds exactly the files
 * the LSH path reads (the reference's own constructor needs more files than that). */
int em2_tool_create_directory(const char* directoryName, uint32_t geneCount, uint32_t cellCount,
                              const uint64_t* toc, const em2_count* data);
int em2_tool_add_gene_set(const char* directoryName, const char* name, const uint32_t* sortedGlobalIds,
                          uint32_t count);
int em2_tool_add_cell_set(const char* directoryName, const char* name, const uint32_t* sortedCellIds,
                          uint32_t count);

/* Writes a Cells file (MemoryMapped::Vector<Cell>, src/Cell.hpp) whose records hold these norm1Inverse / norm2Inverse and
 * zeros elsewhere: one record per global cell. */
int em2_tool_add_cells(const char* directoryName, const double* norm1Inverse, const double* norm2Inverse, uint32_t cellCount);

/* Writes an empty cell meta data store -- one empty list per cell, string tables of the next powers of two at or above the two
 * capacities -- as the reference's ExpressionMatrix constructor and its cellMetaData.push_back() per cell leave one
 * (src/ExpressionMatrix.cpp:81-84, :223). */
int em2_tool_create_meta_data(const char* directoryName, uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity);

/* ---- Ingest ----
 *
 * ExpressionMatrix::createNew (src/ExpressionMatrix.cpp:56-101): a new directory with every file of a store -- GeneNames-*,
 * GeneMetaData.{toc,data,freeSlots}, GeneMetaDataNames-*, GeneMetaDataValues-*, GeneMetaDataNamesUsageCount, Cells, CellNames-*,
 * the CellMetaData* family, CellExpressionCounts.{toc,data} (the toc holds the single 0), CellSet-AllCells and
 * GeneSet-AllGenes-{GlobalIds,LocalIds}, empty -- and the open matrix on it.  It is an error (EM2_ERROR_RUNTIME) if the
 * directory exists.  New string tables start at 4096 slots (the reference: up to 1 << 24) and double as the reference's do;
 * vectors grow by doubling (the reference: 1.5 times).  Every file passes the reference's open checks
 * (src/MemoryMappedVector.hpp:497-499); capacities and file sizes are not the reference's, object counts and objects are.
 *
 * em2_matrix_open opens these files where the directory has them.  On a directory without them (em2_tool_create_directory)
 * every entry below except the two counts fails with EM2_ERROR_RUNTIME and a text that names the missing file.  The string
 * tables and the gene meta data are kept in host memory and written by em2_matrix_flush and em2_matrix_close, as the cell
 * meta data is; the vectors (counts, Cells, AllCells, AllGenes) grow in their mapped files.  After any of the calls every
 * other entry of the same handle sees the new genes and cells. */
int em2_matrix_create(const char* directoryName, em2_matrix** matrix);

/* geneCount() and cellCount() (src/ExpressionMatrix.hpp).  On a directory without GeneNames the gene count is the length of
 * GeneSet-AllGenes-LocalIds. */
int em2_matrix_gene_count(em2_matrix* matrix, uint32_t* geneCount);
int em2_matrix_cell_count(em2_matrix* matrix, uint32_t* cellCount);

/* ExpressionMatrix::addGene (src/ExpressionMatrixGenes.cpp:12-39): *added = 1 and the gene gets the next id, an empty meta
 * data list with the field GeneName, and its place in AllGenes; *added = 0 for a name the store has. */
int em2_matrix_add_gene(em2_matrix* matrix, const char* geneName, int* added);

/* geneName, geneIdFromName and cellIdFromString (src/ExpressionMatrix.cpp:822-874).  The name comes by the two-call protocol
 * of em2_matrix_get_cell_meta_data_value; a gene id not below the gene count is EM2_ERROR_INVALID_ARGUMENT (the reference
 * reads out of bounds).  An unknown name gives 0xffffffff.  cellIdFromString takes a text as a cell id where
 * lexical_cast<CellId> does and the number is below the cell count, and as a cell name otherwise.  Accepted as a number: an
 * optional '+', then decimal digits only, value at most 0xffffffff.  (Departure: boost also takes a leading '-' and negates
 * modulo 2^32; here such a text is a name.) */
int em2_matrix_gene_name(em2_matrix* matrix, uint32_t geneId, uint64_t* bytes, char* value);
int em2_matrix_gene_id_from_name(em2_matrix* matrix, const char* geneName, uint32_t* geneId);
int em2_matrix_cell_id_from_string(em2_matrix* matrix, const char* s, uint32_t* cellId);

/* ExpressionMatrix::addCell (src/ExpressionMatrix.cpp:165-294).  metaData: metaDataPairCount (name, value) pairs as
 * name\0value\0...; geneNames: countCount names, each followed by \0, counts[i] the count of geneNames[i].  CellName is
 * required ("CellName missing from cell meta data.") and moved to the front; "Cell name X already exists."; genes are added
 * as met; a negative count is "Negative expression count encountered."; zeros (and -0.0) are dropped, NaN and inf are stored;
 * sum1 and sum2 are double sums in the caller's order, the square a float product; the kept entries are sorted by gene id;
 * "Duplicate expression count for cell C gene G" names the smallest gene id that two kept entries share.  The last two
 * doubles of the 56-byte Cell record are written as 0 (the reference leaves them uninitialised).
 * Departure: a failing call leaves the store unchanged (the reference leaves a half-added cell). */
int em2_matrix_add_cell(em2_matrix* matrix, const char* metaData, uint64_t metaDataBytes, uint32_t metaDataPairCount,
                        const char* geneNames, uint64_t geneNamesBytes, const float* counts, uint32_t countCount, uint32_t* cellId);

/* The storing part of addCell (src/ExpressionMatrix.cpp:241-277) for cellCount rows of a sparse matrix in device memory, in
 * two passes because the size of the result is not known beforehand.  Row i is d_indices / d_values [d_indptr[i],
 * d_indptr[i + 1]); d_indptr[0] = 0 and every row is shorter than 2^31.  The gene of an entry is
 * d_geneIdOfIndex[d_indices[j]], indexCount the length of that map.  d_skip (may be NULL): rows that are not added --
 * neither counted nor checked.
 *   _count   d_keptCount[i]: the entries that are not zero; d_status[i]: 0 ok, 1 a negative value, 2 two kept entries of one
 *            gene -- d_duplicateGene[i] is then the smallest such gene id, 0xffffffff otherwise -- 3 an index not below
 *            indexCount; a negative value wins over a duplicate.  d_outToc[0..cellCount]: the exclusive sums of d_keptCount.
 *   _fill    the kept entries of every row that is not skipped, ascending by gene id, at d_outData[d_outToc[i]], and the
 *            row's Cell record (7 doubles: sum1, sum2, norm2, 1/sum1, 1/norm2, 0, 0) at d_outCells + 56 i; a skipped row's
 *            record is left as it is.  For rows whose status is 0.  EM2_ERROR_INVALID_ARGUMENT, and nothing written out of
 *            place, if d_outToc is not the one _count gave.
 * sum1, sum2 are the sequential double sums in input order bit for bit; sqrt and the divisions are correctly rounded.  Both
 * calls allocate their own scratch and leave the stream synchronised. */
int em2_dev_ingest_count(const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                         uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, uint32_t* d_keptCount,
                         uint32_t* d_status, uint32_t* d_duplicateGene, uint64_t* d_outToc, void* stream);
int em2_dev_ingest_fill(const uint64_t* d_indptr, const uint32_t* d_indices, const float* d_values, const uint8_t* d_skip,
                        uint32_t cellCount, const uint32_t* d_geneIdOfIndex, uint32_t indexCount, const uint64_t* d_outToc,
                        em2_count* d_outData, void* d_outCells, void* stream);

/* Rows of at most this many entries are sorted in LDS (a wave up to 512 entries, a workgroup above), longer ones in global
 * memory.  0 restores the default, 8192; at most 16384.  For tests. */
void em2_set_ingest_lds_row_limit(uint32_t entries);

/* The per-barcode loop of ExpressionMatrix::addCellsFromHdf5 (src/ExpressionMatrixHdf5.cpp:113-200) on the arrays of the
 * file: every name of geneNames is added (:116-118; a name twice in geneNames is the error of :72-90, "Duplicate gene name X
 * in geneNames"), then every barcode i with skip[i] == 0 (skip may be NULL) becomes the cell cellNamePrefix + "-" +
 * cellNames[i] with the meta data CellName and then the cellMetaData pairs, its counts values[j] of the genes
 * geneNames[indices[j]], j in [indptr[i], indptr[i + 1]).  Strings are packed as for em2_matrix_add_cell.  The cells' entries
 * are prepared on the device (em2_dev_ingest_count, em2_dev_ingest_fill) in chunks of barcodes whose arrays take at most
 * chunkBytes bytes (0: 1 GiB; one barcode at least); names and meta data lists are written on the host, string ids in the
 * reference's order of first insertion.  *firstCellId is the id of the first added cell, *addedCellCount their number.
 * Departures: the call is all or nothing, genes included; the error is that of the lowest failing barcode, within a barcode
 * addCell's order (name exists, negative, duplicate); a skipped barcode is neither named nor checked.  An index not below
 * geneNameCount, an indptr that does not start at 0, descends or does not end at entryCount is EM2_ERROR_INVALID_ARGUMENT
 * before any work (the reference asserts). */
int em2_matrix_add_cells_csr(em2_matrix* matrix, const char* geneNames, uint64_t geneNamesBytes, uint32_t geneNameCount,
                             const char* cellNames, uint64_t cellNamesBytes, uint32_t cellCount, const uint64_t* indptr,
                             const uint32_t* indices, const float* values, uint64_t entryCount, const uint8_t* skip,
                             const char* cellNamePrefix, const char* cellMetaData, uint64_t cellMetaDataBytes,
                             uint32_t cellMetaDataPairCount, uint64_t chunkBytes, uint32_t* firstCellId, uint32_t* addedCellCount);

/* tokenize (src/tokenize.cpp:16-35, boost::escaped_list_separator<char>("\\", separators, "\"")) restated: a '\\' makes the
 * next byte literal ('n' a line feed; a quote, a '\\' or a separator itself; nothing after it is "cannot end with escape",
 * anything else "unknown escape sequence", both EM2_ERROR_RUNTIME); a separator byte outside quotes ends the token; '"'
 * toggles the quote state and is dropped, an open quote at the end is no error; an empty line has no token, a line ending in
 * a separator a last empty one.  With removeLeadingAndTrailingBlanks every token is trimmed of space, \t, \n, \v, \f, \r.
 * The tokens come back each followed by NUL: call with packed == NULL for *bytes, then with a buffer of that size. */
int em2_csv_tokenize(const char* separators, const char* line, uint64_t lineBytes, int removeLeadingAndTrailingBlanks, uint64_t* tokenCount,
                     uint64_t* bytes, char* packed);

/* The per-line work of ExpressionMatrix::addCells (src/ExpressionMatrix.cpp:559-626: getline, tokenize, the "0" / "0." test
 * and strtof of every kept field) for a chunk of whole lines in device memory.  d_text need not be aligned; textBytes is at
 * most 0xf0000000.  separators: 1 to 8 bytes in host memory, none of them '"', '\\', '\n', '\r' or NUL.  Lines are getline's:
 * split at '\n' whatever the quotes say, a last line without '\n' counts.
 *   d_lineTable[6 i ..]   of line i: begin, end (offsets into the text, the '\n' and one '\r' before it excluded), token count,
 *                         status, begin and end of the first field.  Status 0 ok; 1 the line is empty (before the '\r' is
 *                         removed); 2 the token count is not expectedTokens; 3 the line holds a '\\': the device reports its
 *                         begin and end and nothing else, the host tokenizes it whole.
 *   triples               for every field of a column c < expectedTokens with d_keptCellOfColumn[c] != 0xffffffff, in a line
 *                         without '\\', that the device decides and that is not skipped: key = kept cell << 32 | (lineBase +
 *                         i), value = strtof's float.  In no particular order.
 *   d_deferred[4 j ..]    the fields of such columns the device does not decide: lineBase + i, column, begin, end.  Likewise.
 * Decided: a field without '"' whose trimmed text is "0" or "0." is skipped, as the reference skips it; one that matches
 * [+-]?(D+(\.D*)?|\.D+)([eE][+-]?D+)? in at most 32 bytes, with at most 19 digits from the first that is not 0 (an exact
 * uint64 m), m <= 2^53, at most 4 exponent digits and |q| <= 22 for q = exponent - fraction digits, has the value
 * float(d), d = double(m) * 10^q or double(m) / 10^-q: one correctly rounded operation on exact operands, so d is the double
 * nearest the field's value x.  strtof is correctly rounded; if float(d) were not the float nearest x, a float rounding
 * midpoint M would lie between x and d inclusive, M is a double, so M would be as near to x as d is: M = d.  A d whose low 29
 * significand bits are exactly 1 << 28 is such a midpoint and is deferred, as is a d != 0 outside the normal float range.
 * Everything else is deferred: quotes, longer fields, hex, inf, nan, trailing text, empty fields.  Unkept columns are not read.
 * counts[0..2] (host): the lines, the triples, the deferred fields of the text.  Where counts[0] > lineCapacity nothing else
 * was written; where counts[1] or counts[2] exceed their capacity the list holds its first `capacity` elements: call again
 * with room.  Allocates its own scratch and leaves the stream synchronised. */
int em2_dev_csv_parse(const char* d_text, uint64_t textBytes, const char* separators, uint32_t separatorCount, uint32_t expectedTokens,
                      const uint32_t* d_keptCellOfColumn, uint32_t lineBase, uint32_t lineCapacity, uint32_t* d_lineTable,
                      uint64_t tripleCapacity, uint64_t* d_tripleKeys, float* d_tripleValues, uint64_t deferredCapacity,
                      uint32_t* d_deferred, uint64_t* counts, void* stream);

/* The text is read in tiles of this many bytes (rounded up to 16; at most 1 MiB) when its lines are counted and placed; 0
 * restores the default, 16384.  For tests: a 2 KB text then spans many tiles. */
void em2_set_csv_tile_bytes(uint32_t bytes);

/* ExpressionMatrix::addCells (src/ExpressionMatrix.cpp:380-654): the cells that both files name, in the order of the
 * expression counts file's columns (the loop of :535-543), each with additionalCellMetaData, then CellName, then the fields
 * of the meta data file (addCell then swaps the first CellName pair to the front, :190-197).  The meta data file is
 * tokenized without trimming, the expression counts file with; either header may have one token fewer than the second line;
 * every gene line adds its gene; an unkept column is never parsed.  The reference's order of checks and error texts.  The
 * expression counts file goes to the device in chunks of whole lines of at most chunkBytes bytes (0: 256 MiB; a line at
 * least), em2_dev_csv_parse; its counts are sorted by (cell, line) there and stored by em2_dev_ingest_count / _fill.  Lines
 * with a '\\' and deferred fields are resolved on the host.  useDevice == 0, a separator string the device does not take
 * (longer than 8 bytes, or with '"', '\\', '\n', '\r'), or a line of 0xf0000000 bytes: the whole file takes the host path,
 * same result.  *deferredFieldCount (may be NULL): the fields the device deferred.
 * Departures: all or nothing, genes included; a parse error (file order; within a line token count, duplicate gene, first
 * invalid count in kept order) comes before any addCell error, which is that of the lowest failing cell; no progress lines;
 * an empty second line is "Empty line in ... file F" (the reference reads line[-1]). */
int em2_matrix_add_cells_csv(em2_matrix* matrix, const char* expressionCountsFileName, const char* expressionCountsFileSeparators,
                             const char* cellMetaDataFileName, const char* cellMetaDataFileSeparators, const char* additionalCellMetaData,
                             uint64_t additionalCellMetaDataBytes, uint32_t additionalCellMetaDataPairCount, uint64_t chunkBytes,
                             int useDevice, uint32_t* firstCellId, uint32_t* addedCellCount, uint64_t* deferredFieldCount);

/* ExpressionMatrix::addCellMetaData (src/ExpressionMatrixBioHub.cpp:337-392): separator ",", trimmed tokens, no '\r'
 * handling; the first header token is ignored, an empty header name skips its column; "Unexpected number of meta data values
 * in F", "Attempt to add meta data for undefined cell X"; setCellMetaData per (cell, field) in file order.  Host only.
 * Departure: all or nothing (the reference keeps the lines before the failing one). */
int em2_matrix_add_cell_meta_data_csv(em2_matrix* matrix, const char* cellMetaDataFileName);

#ifdef __cplusplus
}
#endif

#endif
