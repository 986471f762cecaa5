// em2_matrix_capi.cpp -- C ABI of the ExpressionMatrix-level entry points (include/em2_lsh.h): translates
// em2::host::Error into status codes + em2_last_error().
#include "em2_host.h"
#include "em2_meta_data.h"
#include "em2_csv.h"

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <string>

// Defined in em2_capi.hip.
extern "C" void em2_internal_set_last_error(const char* message);

struct em2_matrix {
    em2::host::Matrix* impl;
};

struct em2_meta_data_table {
    em2::host::MetaDataTable table;
};

namespace {

template <class F> int guarded(F f)
{
    try {
        f();
        return EM2_OK;
    } catch (const em2::host::Error& e) {
        em2_internal_set_last_error(e.message.c_str());
        return e.code;
    } catch (const std::bad_alloc&) {
        em2_internal_set_last_error("out of host memory");
        return EM2_ERROR_RUNTIME;
    } catch (const std::exception& e) {
        em2_internal_set_last_error(e.what());
        return EM2_ERROR_RUNTIME;
    }
}

int nullArgument(const char* function)
{
    em2_internal_set_last_error((std::string(function) + ": null argument").c_str());
    return EM2_ERROR_INVALID_ARGUMENT;
}

// The set operations' "false": EM2_OK, *created = 0 and the reference's line as the last error.
template <class F> int geneSetOperation(int* created, F f)
{
    *created = 0;
    return guarded([&] {
        std::string message;
        *created = f(message) ? 1 : 0;
        if (!*created) em2_internal_set_last_error(message.c_str());
    });
}

// The two-call protocol of the entries that return bytes: value == NULL asks for *bytes, else *bytes is the buffer's size.
void copyOut(const char* who, const std::string& from, uint64_t* bytes, char* to)
{
    if (to) {
        if (*bytes < from.size()) throw em2::host::Error{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the buffer is too small"};
        if (!from.empty()) std::memcpy(to, from.data(), from.size());
    }
    *bytes = from.size();
}

}  // namespace

extern "C" {

int em2_matrix_open(const char* directoryName, em2_matrix** matrix)
{
    if (!directoryName || !matrix) return nullArgument("em2_matrix_open");
    *matrix = nullptr;
    return guarded([&] {
        em2::host::Matrix* m = new em2::host::Matrix(directoryName);
        *matrix = new em2_matrix{m};
    });
}

void em2_matrix_close(em2_matrix* matrix)
{
    if (matrix) {
        delete matrix->impl;
        delete matrix;
    }
}

int em2_matrix_find_similar_pairs4(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* similarPairsName, size_t k, double similarityThreshold,
                                   size_t lshCount, unsigned int seed)
{
    if (!matrix || !geneSetName || !cellSetName || !similarPairsName) return nullArgument("em2_matrix_find_similar_pairs4");
    return guarded([&] {
        matrix->impl->findSimilarPairs4(geneSetName, cellSetName, similarPairsName, k, similarityThreshold, lshCount, seed);
    });
}

int em2_matrix_compute_lsh_signatures(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                      const char* lshName, size_t lshCount, unsigned int seed)
{
    if (!matrix || !geneSetName || !cellSetName || !lshName) return nullArgument("em2_matrix_compute_lsh_signatures");
    return guarded([&] { matrix->impl->computeLshSignatures(geneSetName, cellSetName, lshName, lshCount, seed); });
}

int em2_matrix_analyze_lsh(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, size_t lshCount,
                           unsigned int seed, double csvDownsample, const char* outputDirectory)
{
    if (!matrix || !geneSetName || !cellSetName) return nullArgument("em2_matrix_analyze_lsh");
    return guarded([&] {
        matrix->impl->analyzeLsh(geneSetName, cellSetName, lshCount, seed, csvDownsample, outputDirectory ? outputDirectory : "");
    });
}

int em2_matrix_create_signature_graph(em2_matrix* matrix, const char* cellSetName, const char* lshName, uint64_t minCellCount,
                                      em2_signature_graph** graph)
{
    if (!matrix || !cellSetName || !lshName || !graph) return nullArgument("em2_matrix_create_signature_graph");
    *graph = nullptr;
    return guarded([&] { matrix->impl->createSignatureGraph(cellSetName, lshName, minCellCount, graph); });
}

int em2_matrix_analyze_lsh_signatures(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, size_t lshCount,
                                      unsigned int seed, const char* outputDirectory)
{
    if (!matrix || !geneSetName || !cellSetName) return nullArgument("em2_matrix_analyze_lsh_signatures");
    return guarded([&] {
        matrix->impl->analyzeLshSignatures(geneSetName, cellSetName, lshCount, seed, outputDirectory ? outputDirectory : "");
    });
}

int em2_matrix_create_gene_graph(em2_matrix* matrix, const char* geneSetName, const char* similarGenePairsName, int64_t k,
                                 double similarityThreshold, em2_gene_graph** graph)
{
    if (!matrix || !geneSetName || !similarGenePairsName || !graph) return nullArgument("em2_matrix_create_gene_graph");
    *graph = nullptr;
    return guarded([&] { matrix->impl->createGeneGraph(geneSetName, similarGenePairsName, k, similarityThreshold, graph); });
}

int em2_matrix_create_gene_set_intersection(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName, int* created)
{
    if (!matrix || !inputSetsNames || !outputSetName || !created) return nullArgument("em2_matrix_create_gene_set_intersection");
    return geneSetOperation(created, [&](std::string& message) {
        return matrix->impl->createGeneSetIntersectionOrUnion(inputSetsNames, outputSetName, false, message);
    });
}

int em2_matrix_create_gene_set_union(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName, int* created)
{
    if (!matrix || !inputSetsNames || !outputSetName || !created) return nullArgument("em2_matrix_create_gene_set_union");
    return geneSetOperation(created, [&](std::string& message) {
        return matrix->impl->createGeneSetIntersectionOrUnion(inputSetsNames, outputSetName, true, message);
    });
}

int em2_matrix_create_gene_set_difference(em2_matrix* matrix, const char* inputSetName0, const char* inputSetName1,
                                          const char* outputSetName, int* created)
{
    if (!matrix || !inputSetName0 || !inputSetName1 || !outputSetName || !created) return nullArgument("em2_matrix_create_gene_set_difference");
    return geneSetOperation(created, [&](std::string& message) {
        return matrix->impl->createGeneSetDifference(inputSetName0, inputSetName1, outputSetName, message);
    });
}

int em2_matrix_find_similar_pairs5(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, size_t lshSliceLength, size_t bucketOverflow)
{
    if (!matrix || !geneSetName || !cellSetName || !lshName || !similarPairsName) return nullArgument("em2_matrix_find_similar_pairs5");
    return guarded([&] {
        matrix->impl->findSimilarPairs5(geneSetName, cellSetName, lshName, similarPairsName, k, similarityThreshold,
                                        lshSliceLength, bucketOverflow);
    });
}

int em2_matrix_find_similar_pairs6(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, size_t permutationCount, size_t searchCount,
                                   size_t permutedBitCount, int seed)
{
    if (!matrix || !geneSetName || !cellSetName || !lshName || !similarPairsName) return nullArgument("em2_matrix_find_similar_pairs6");
    return guarded([&] {
        matrix->impl->findSimilarPairs6(geneSetName, cellSetName, lshName, similarPairsName, k, similarityThreshold,
                                        permutationCount, searchCount, permutedBitCount, seed);
    });
}

int em2_matrix_find_similar_pairs7(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* lshName, const char* similarPairsName, size_t k,
                                   double similarityThreshold, const int32_t* lshSliceLengths, uint32_t sliceLengthCount,
                                   uint32_t maxCheck, size_t log2BucketCount)
{
    if (!matrix || !geneSetName || !cellSetName || !lshName || !similarPairsName || (!lshSliceLengths && sliceLengthCount)) {
        return nullArgument("em2_matrix_find_similar_pairs7");
    }
    return guarded([&] {
        matrix->impl->findSimilarPairs7(geneSetName, cellSetName, lshName, similarPairsName, k, similarityThreshold,
                                        std::vector<int32_t>(lshSliceLengths, lshSliceLengths + sliceLengthCount), maxCheck,
                                        log2BucketCount);
    });
}

int em2_matrix_find_similar_pairs0(em2_matrix* matrix, const char* geneSetName, const char* cellSetName,
                                   const char* similarPairsName, size_t k, double similarityThreshold)
{
    if (!matrix || !geneSetName || !cellSetName || !similarPairsName) return nullArgument("em2_matrix_find_similar_pairs0");
    return guarded([&] { matrix->impl->findSimilarPairs0(geneSetName, cellSetName, similarPairsName, k, similarityThreshold); });
}

int em2_matrix_analyze_similar_pairs(em2_matrix* matrix, const char* similarPairsName, double csvDownsample,
                                     const char* outputDirectory)
{
    if (!matrix || !similarPairsName) return nullArgument("em2_matrix_analyze_similar_pairs");
    return guarded([&] { matrix->impl->analyzeSimilarPairs(similarPairsName, csvDownsample, outputDirectory ? outputDirectory : ""); });
}

int em2_matrix_compute_cell_similarity(em2_matrix* matrix, const char* geneSetName, uint32_t cellId0, uint32_t cellId1,
                                       double* similarity)
{
    if (!matrix || !geneSetName || !similarity) return nullArgument("em2_matrix_compute_cell_similarity");
    return guarded([&] { *similarity = matrix->impl->computeCellSimilarity(geneSetName, cellId0, cellId1); });
}

int em2_matrix_cell_similarities_to_cell(em2_matrix* matrix, const char* geneSetName, uint32_t cellId0, const uint32_t* cellIds, uint32_t count,
                                         double* out)
{
    if (!matrix || !geneSetName || (count && (!cellIds || !out))) return nullArgument("em2_matrix_cell_similarities_to_cell");
    return guarded([&] { matrix->impl->cellSimilaritiesToCell(geneSetName, cellId0, cellIds, count, out); });
}

int em2_matrix_gene_expression_of_cells(em2_matrix* matrix, const char* geneSetName, uint32_t globalGeneId, int normalizationMethod,
                                        const uint32_t* cellIds, uint32_t count, float* out)
{
    if (!matrix || !geneSetName || (count && (!cellIds || !out))) return nullArgument("em2_matrix_gene_expression_of_cells");
    return guarded([&] { matrix->impl->geneExpressionOfCells(geneSetName, globalGeneId, normalizationMethod, cellIds, count, out); });
}

int em2_matrix_compare_similar_pairs(em2_matrix* matrix, const char* similarPairsName0, const char* similarPairsName1,
                                     const char* outputDirectory)
{
    if (!matrix || !similarPairsName0 || !similarPairsName1) return nullArgument("em2_matrix_compare_similar_pairs");
    return guarded([&] { matrix->impl->compareSimilarPairs(similarPairsName0, similarPairsName1, outputDirectory ? outputDirectory : ""); });
}

int em2_matrix_remove_similar_pairs(em2_matrix* matrix, const char* similarPairsName)
{
    if (!matrix || !similarPairsName) return nullArgument("em2_matrix_remove_similar_pairs");
    return guarded([&] { matrix->impl->removeSimilarPairs(similarPairsName); });
}

int em2_matrix_find_similar_gene_pairs0(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                        const char* similarGenePairsName, size_t k, double similarityThreshold)
{
    if (!matrix || !geneSetName || !cellSetName || !similarGenePairsName) return nullArgument("em2_matrix_find_similar_gene_pairs0");
    return guarded([&] {
        matrix->impl->findSimilarGenePairs0(geneSetName, cellSetName, normalizationMethod, similarGenePairsName, k, similarityThreshold);
    });
}

int em2_matrix_remove_similar_gene_pairs(em2_matrix* matrix, const char* similarGenePairsName)
{
    if (!matrix || !similarGenePairsName) return nullArgument("em2_matrix_remove_similar_gene_pairs");
    return guarded([&] { matrix->impl->removeSimilarGenePairs(similarGenePairsName); });
}

int em2_matrix_gene_information_content(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                        float* out)
{
    if (!matrix || !geneSetName || !cellSetName) return nullArgument("em2_matrix_gene_information_content");
    return guarded([&] {
        std::vector<float> informationContent;
        matrix->impl->geneInformation(geneSetName, cellSetName, normalizationMethod, &informationContent, nullptr);
        if (!informationContent.empty()) {
            if (!out) throw em2::host::Error{EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_gene_information_content: null argument"};
            std::memcpy(out, informationContent.data(), informationContent.size() * sizeof(float));
        }
    });
}

int em2_matrix_rank_genes(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                          const uint32_t* group, uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2,
                          uint64_t* tieSum, double* zScore, double* auc)
{
    if (!matrix || !geneSetName || !cellSetName) return nullArgument("em2_matrix_rank_genes");
    return guarded([&] {
        matrix->impl->rankGenes(geneSetName, cellSetName, normalizationMethod, group, groupCount, groupSize, nonZeroCount, rankSum2,
                                tieSum, zScore, auc);
    });
}

int em2_matrix_create_gene_set_using_information_content(em2_matrix* matrix, const char* existingGeneSetName, const char* cellSetName,
                                                         int normalizationMethod, double geneInformationContentThreshold,
                                                         const char* newGeneSetName)
{
    if (!matrix || !existingGeneSetName || !cellSetName || !newGeneSetName) {
        return nullArgument("em2_matrix_create_gene_set_using_information_content");
    }
    return guarded([&] {
        matrix->impl->createGeneSetUsingInformationContent(existingGeneSetName, cellSetName, normalizationMethod,
                                                           geneInformationContentThreshold, newGeneSetName);
    });
}

int em2_matrix_create_well_expressed_gene_set(em2_matrix* matrix, const char* inputGeneSetName, const char* inputCellSetName,
                                              const char* outputGeneSetName, uint32_t minCellCount)
{
    if (!matrix || !inputGeneSetName || !inputCellSetName || !outputGeneSetName) return nullArgument("em2_matrix_create_well_expressed_gene_set");
    return guarded([&] { matrix->impl->createWellExpressedGeneSet(inputGeneSetName, inputCellSetName, outputGeneSetName, minCellCount); });
}

int em2_matrix_remove_gene_set(em2_matrix* matrix, const char* geneSetName)
{
    if (!matrix || !geneSetName) return nullArgument("em2_matrix_remove_gene_set");
    return guarded([&] { matrix->impl->removeGeneSet(geneSetName); });
}

int em2_matrix_create_cell_set(em2_matrix* matrix, const char* cellSetName, const uint32_t* cellIds, uint32_t count)
{
    if (!matrix || !cellSetName || (!cellIds && count)) return nullArgument("em2_matrix_create_cell_set");
    return guarded([&] { matrix->impl->createCellSet(cellSetName, std::vector<uint32_t>(cellIds, cellIds + count)); });
}

int em2_matrix_create_cell_set_intersection(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName)
{
    if (!matrix || !inputSetsNames || !outputSetName) return nullArgument("em2_matrix_create_cell_set_intersection");
    return guarded([&] { matrix->impl->createCellSetIntersectionOrUnion(inputSetsNames, outputSetName, false); });
}

int em2_matrix_create_cell_set_union(em2_matrix* matrix, const char* inputSetsNames, const char* outputSetName)
{
    if (!matrix || !inputSetsNames || !outputSetName) return nullArgument("em2_matrix_create_cell_set_union");
    return guarded([&] { matrix->impl->createCellSetIntersectionOrUnion(inputSetsNames, outputSetName, true); });
}

int em2_matrix_create_cell_set_difference(em2_matrix* matrix, const char* inputSetName0, const char* inputSetName1,
                                          const char* outputSetName)
{
    if (!matrix || !inputSetName0 || !inputSetName1 || !outputSetName) return nullArgument("em2_matrix_create_cell_set_difference");
    return guarded([&] { matrix->impl->createCellSetDifference(inputSetName0, inputSetName1, outputSetName); });
}

int em2_matrix_downsample_cell_set(em2_matrix* matrix, const char* inputCellSetName, const char* outputCellSetName, double probability,
                                   int seed)
{
    if (!matrix || !inputCellSetName || !outputCellSetName) return nullArgument("em2_matrix_downsample_cell_set");
    return guarded([&] { matrix->impl->downsampleCellSet(inputCellSetName, outputCellSetName, probability, seed); });
}

int em2_matrix_remove_cell_set(em2_matrix* matrix, const char* cellSetName)
{
    if (!matrix || !cellSetName) return nullArgument("em2_matrix_remove_cell_set");
    return guarded([&] { matrix->impl->removeCellSet(cellSetName); });
}

int em2_matrix_cell_set_names(em2_matrix* matrix, uint64_t* bytes, char* names)
{
    if (!matrix || !bytes) return nullArgument("em2_matrix_cell_set_names");
    return guarded([&] {
        std::string all;
        for (const std::string& name : matrix->impl->cellSetNames()) all.append(name).push_back('\0');
        if (names) {
            if (*bytes < all.size()) throw em2::host::Error{EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_cell_set_names: the buffer is too small"};
            std::memcpy(names, all.data(), all.size());
        }
        *bytes = all.size();
    });
}

int em2_matrix_dense_expression(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, int normalizationMethod,
                                int elementType, uint32_t rowBegin, uint32_t rowEnd, void* out)
{
    if (!matrix || !geneSetName || !cellSetName) return nullArgument("em2_matrix_dense_expression");
    return guarded([&] {
        matrix->impl->denseExpression(geneSetName, cellSetName, normalizationMethod, elementType, rowBegin, rowEnd, out);
    });
}

int em2_matrix_cell_expression_counts(em2_matrix* matrix, uint32_t cellId, uint64_t* count, em2_count* out)
{
    if (!matrix || !count) return nullArgument("em2_matrix_cell_expression_counts");
    return guarded([&] {
        const em2_count* entries = nullptr;
        uint64_t stored = 0;
        matrix->impl->cellExpressionCounts(cellId, entries, stored);
        if (out) {
            if (*count < stored) throw em2::host::Error{EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_cell_expression_counts: the buffer is too small"};
            if (stored) std::memcpy(out, entries, stored * sizeof(em2_count));
        }
        *count = stored;
    });
}

int em2_similar_gene_pairs_write(const char* directoryName, const char* similarGenePairsName, const char* geneSetName,
                                 const char* cellSetName, size_t k, int normalizationMethod, uint32_t geneCount, const em2_pair* pairs,
                                 const uint32_t* usedCount)
{
    if (!directoryName || !similarGenePairsName || !geneSetName || !cellSetName || (!usedCount && geneCount) || (!pairs && k && geneCount)) {
        return nullArgument("em2_similar_gene_pairs_write");
    }
    return guarded([&] {
        em2::host::writeSimilarGenePairs(directoryName, similarGenePairsName, geneSetName, cellSetName, k, normalizationMethod, geneCount,
                                         pairs, usedCount);
    });
}

int em2_similar_gene_pairs_read(const char* directoryName, const char* similarGenePairsName, uint64_t* k, uint64_t* geneCount,
                                int* normalizationMethod, char* geneSetName, char* cellSetName, uint64_t* geneSetHash,
                                uint64_t* cellSetHash, em2_pair* pairs, uint32_t* usedCount)
{
    if (!directoryName || !similarGenePairsName || !k || !geneCount) return nullArgument("em2_similar_gene_pairs_read");
    return guarded([&] {
        em2::host::SimilarGenePairsInfo info;
        std::vector<em2_pair> p;
        std::vector<uint32_t> u;
        em2::host::readSimilarGenePairs(directoryName, similarGenePairsName, info, pairs ? &p : nullptr, usedCount ? &u : nullptr);
        *k = info.k;
        *geneCount = info.geneCount;
        if (normalizationMethod) *normalizationMethod = info.normalizationMethod;
        if (geneSetHash) *geneSetHash = info.geneSetHash;
        if (cellSetHash) *cellSetHash = info.cellSetHash;
        if (geneSetName) {
            std::memset(geneSetName, 0, 256);
            std::memcpy(geneSetName, info.geneSetName.data(), info.geneSetName.size());
        }
        if (cellSetName) {
            std::memset(cellSetName, 0, 256);
            std::memcpy(cellSetName, info.cellSetName.data(), info.cellSetName.size());
        }
        if (pairs && !p.empty()) std::memcpy(pairs, p.data(), p.size() * sizeof(em2_pair));
        if (usedCount && !u.empty()) std::memcpy(usedCount, u.data(), u.size() * sizeof(uint32_t));
    });
}

int em2_matrix_subset(em2_matrix* matrix, const char* geneSetName, const char* cellSetName, uint32_t* geneCount,
                      uint32_t* cellCount, uint64_t* nnz, uint64_t* toc, em2_count* data)
{
    if (!matrix || !geneSetName || !cellSetName || !geneCount || !cellCount || !nnz) return nullArgument("em2_matrix_subset");
    return guarded([&] {
        std::vector<uint64_t> t;
        std::vector<em2_count> d;
        matrix->impl->subset(geneSetName, cellSetName, t, d, *geneCount, *cellCount);
        *nnz = d.size();
        if (toc) {
            std::memcpy(toc, t.data(), t.size() * sizeof(uint64_t));
            if (!d.empty() && data) std::memcpy(data, d.data(), d.size() * sizeof(em2_count));
        }
    });
}

int em2_similar_pairs_write(const char* directoryName, const char* similarPairsName, const char* geneSetName,
                            const char* cellSetName, size_t k, uint32_t cellCount, const em2_pair* pairs,
                            const uint32_t* usedCount)
{
    if (!directoryName || !similarPairsName || !geneSetName || !cellSetName || !usedCount || (!pairs && k && cellCount)) {
        return nullArgument("em2_similar_pairs_write");
    }
    return guarded([&] {
        em2::host::writeSimilarPairs(directoryName, similarPairsName, geneSetName, cellSetName, k, cellCount, pairs, usedCount);
    });
}

int em2_similar_pairs_read(const char* directoryName, const char* similarPairsName, uint64_t* k,
                           uint64_t* cellCount, em2_pair* pairs, uint32_t* usedCount)
{
    if (!directoryName || !similarPairsName || !k || !cellCount) return nullArgument("em2_similar_pairs_read");
    return guarded([&] {
        em2::host::SimilarPairsInfo info;
        std::vector<em2_pair> p;
        std::vector<uint32_t> u;
        em2::host::readSimilarPairs(directoryName, similarPairsName, info, pairs ? &p : nullptr, usedCount ? &u : nullptr);
        *k = info.k;
        *cellCount = info.cellCount;
        if (pairs && !p.empty()) std::memcpy(pairs, p.data(), p.size() * sizeof(em2_pair));
        if (usedCount && !u.empty()) std::memcpy(usedCount, u.data(), u.size() * sizeof(uint32_t));
    });
}

int em2_similar_pairs_info(const char* directoryName, const char* similarPairsName, uint64_t* k, uint64_t* cellCount,
                           char* geneSetName, char* cellSetName)
{
    if (!directoryName || !similarPairsName || !k || !cellCount || !geneSetName || !cellSetName) return nullArgument("em2_similar_pairs_info");
    return guarded([&] {
        em2::host::SimilarPairsInfo info;
        em2::host::readSimilarPairs(directoryName, similarPairsName, info, nullptr, nullptr);
        *k = info.k;
        *cellCount = info.cellCount;
        std::memset(geneSetName, 0, 256);
        std::memset(cellSetName, 0, 256);
        std::memcpy(geneSetName, info.geneSetName.data(), info.geneSetName.size());
        std::memcpy(cellSetName, info.cellSetName.data(), info.cellSetName.size());
    });
}

int em2_matrix_cell_set(em2_matrix* matrix, const char* cellSetName, uint32_t* count, uint32_t* ids)
{
    if (!matrix || !cellSetName || !count) return nullArgument("em2_matrix_cell_set");
    return guarded([&] {
        const em2::host::MappedFile& f = matrix->impl->cellSet(cellSetName);
        *count = uint32_t(f.objectCount());
        if (ids && *count) std::memcpy(ids, f.data(), size_t(*count) * sizeof(uint32_t));
    });
}

int em2_matrix_gene_set(em2_matrix* matrix, const char* geneSetName, uint32_t* count, uint32_t* globalIds)
{
    if (!matrix || !geneSetName || !count) return nullArgument("em2_matrix_gene_set");
    return guarded([&] {
        const em2::host::GeneSet& g = matrix->impl->geneSet(geneSetName);
        *count = g.size();
        if (globalIds && *count) std::memcpy(globalIds, g.genes(), size_t(*count) * sizeof(uint32_t));
    });
}

int em2_lsh_write(const char* directoryName, const char* lshName, uint64_t cellCount, uint64_t lshCount,
                  const uint64_t* signatures)
{
    if (!directoryName || !lshName || (!signatures && cellCount) || lshCount == 0) return nullArgument("em2_lsh_write");
    return guarded([&] {
        em2::host::writeLsh(std::string(directoryName) + "/Lsh-" + lshName, cellCount, lshCount, signatures);
    });
}

int em2_lsh_read(const char* directoryName, const char* lshName, uint64_t* cellCount, uint64_t* lshCount,
                 uint64_t* signatures)
{
    if (!directoryName || !lshName || !cellCount || !lshCount) return nullArgument("em2_lsh_read");
    return guarded([&] {
        const std::string prefix = std::string(directoryName) + "/Lsh-" + lshName;
        if (!signatures) {
            em2::host::readLshInfo(prefix, *cellCount, *lshCount);
        } else {
            std::vector<uint64_t> s;
            em2::host::readLsh(prefix, *cellCount, *lshCount, s);
            if (!s.empty()) std::memcpy(signatures, s.data(), s.size() * sizeof(uint64_t));
        }
    });
}

int em2_tool_create_directory(const char* directoryName, uint32_t geneCount, uint32_t cellCount,
                              const uint64_t* toc, const em2_count* data)
{
    if (!directoryName || !toc) return nullArgument("em2_tool_create_directory");
    return guarded([&] { em2::host::createDirectoryFromCsr(directoryName, geneCount, cellCount, toc, data); });
}

int em2_tool_add_gene_set(const char* directoryName, const char* name, const uint32_t* sortedGlobalIds, uint32_t count)
{
    if (!directoryName || !name || (!sortedGlobalIds && count)) return nullArgument("em2_tool_add_gene_set");
    return guarded([&] { em2::host::addGeneSet(directoryName, name, sortedGlobalIds, count, 0); });
}

int em2_tool_add_cell_set(const char* directoryName, const char* name, const uint32_t* sortedCellIds, uint32_t count)
{
    if (!directoryName || !name || (!sortedCellIds && count)) return nullArgument("em2_tool_add_cell_set");
    return guarded([&] { em2::host::addCellSet(directoryName, name, sortedCellIds, count); });
}

int em2_tool_add_cells(const char* directoryName, const double* norm1Inverse, const double* norm2Inverse, uint32_t cellCount)
{
    if (!directoryName || ((!norm1Inverse || !norm2Inverse) && cellCount)) return nullArgument("em2_tool_add_cells");
    return guarded([&] { em2::host::addCells(directoryName, norm1Inverse, norm2Inverse, cellCount); });
}

// ---- cell meta data (em2_meta_data.cpp) ----

int em2_matrix_set_cell_meta_data(em2_matrix* matrix, uint32_t cellId, const char* name, const char* value)
{
    if (!matrix || !name || !value) return nullArgument("em2_matrix_set_cell_meta_data");
    return guarded([&] { matrix->impl->setCellMetaData(cellId, name, value); });
}

int em2_matrix_get_cell_meta_data_value(em2_matrix* matrix, uint32_t cellId, const char* metaDataName, uint64_t* bytes, char* value)
{
    if (!matrix || !metaDataName || !bytes) return nullArgument("em2_matrix_get_cell_meta_data_value");
    return guarded([&] { copyOut("em2_matrix_get_cell_meta_data_value", matrix->impl->cellMetaDataValue(cellId, metaDataName), bytes, value); });
}

int em2_matrix_get_cell_meta_data(em2_matrix* matrix, uint32_t cellId, uint64_t* bytes, char* pairs)
{
    if (!matrix || !bytes) return nullArgument("em2_matrix_get_cell_meta_data");
    return guarded([&] {
        std::string all;
        for (const auto& p : matrix->impl->cellMetaData(cellId)) {
            all.append(p.first).push_back('\0');
            all.append(p.second).push_back('\0');
        }
        copyOut("em2_matrix_get_cell_meta_data", all, bytes, pairs);
    });
}

int em2_matrix_remove_cell_meta_data(em2_matrix* matrix, const char* cellSetName, const char* metaDataName)
{
    if (!matrix || !cellSetName || !metaDataName) return nullArgument("em2_matrix_remove_cell_meta_data");
    return guarded([&] { matrix->impl->removeCellMetaData(cellSetName, metaDataName); });
}

int em2_matrix_create_cell_set_using_meta_data(em2_matrix* matrix, const char* cellSetName, const char* metaDataFieldName,
                                               const char* matchString, int useRegex)
{
    if (!matrix || !cellSetName || !metaDataFieldName || !matchString) return nullArgument("em2_matrix_create_cell_set_using_meta_data");
    return guarded([&] { matrix->impl->createCellSetUsingMetaData(cellSetName, metaDataFieldName, matchString, useRegex != 0); });
}

int em2_matrix_compute_meta_data_rand_index(em2_matrix* matrix, const char* cellSetName, const char* metaDataName0,
                                            const char* metaDataName1, double* randIndex, double* adjustedRandIndex)
{
    if (!matrix || !cellSetName || !metaDataName0 || !metaDataName1 || !randIndex || !adjustedRandIndex) {
        return nullArgument("em2_matrix_compute_meta_data_rand_index");
    }
    return guarded([&] { matrix->impl->computeMetaDataRandIndex(cellSetName, metaDataName0, metaDataName1, *randIndex, *adjustedRandIndex); });
}

int em2_matrix_meta_data_table(em2_matrix* matrix, const char* cellSetName, const char* metaDataName0, const char* metaDataName1,
                               em2_meta_data_table** table)
{
    if (!matrix || !cellSetName || !metaDataName0 || !table) return nullArgument("em2_matrix_meta_data_table");
    *table = nullptr;
    return guarded([&] {
        std::unique_ptr<em2_meta_data_table> t(new em2_meta_data_table);
        const std::string name1 = metaDataName1 ? metaDataName1 : "";
        matrix->impl->metaDataTable(cellSetName, metaDataName0, metaDataName1 ? &name1 : nullptr, t->table);
        *table = t.release();
    });
}

int em2_meta_data_table_sizes(const em2_meta_data_table* table, uint64_t* valueCount0, uint64_t* valueCount1, uint64_t* valueBytes0,
                              uint64_t* valueBytes1, uint64_t* nonZeroCount, int* path)
{
    if (!table) return nullArgument("em2_meta_data_table_sizes");
    const em2::host::MetaDataTable& t = table->table;
    uint64_t bytes[2] = {0, 0};
    for (int f = 0; f < 2; f++) {
        for (const std::string& value : t.values[f]) bytes[f] += value.size() + 1u;
    }
    if (valueCount0) *valueCount0 = t.values[0].size();
    if (valueCount1) *valueCount1 = t.values[1].size();
    if (valueBytes0) *valueBytes0 = bytes[0];
    if (valueBytes1) *valueBytes1 = bytes[1];
    if (nonZeroCount) *nonZeroCount = t.count.size();
    if (path) *path = t.path;
    return EM2_OK;
}

int em2_meta_data_table_get(const em2_meta_data_table* table, char* values0, uint64_t* counts0, char* values1, uint64_t* counts1,
                            uint64_t* row, uint64_t* column, uint64_t* count, uint64_t* sums)
{
    if (!table) return nullArgument("em2_meta_data_table_get");
    const em2::host::MetaDataTable& t = table->table;
    char* values[2] = {values0, values1};
    uint64_t* counts[2] = {counts0, counts1};
    for (int f = 0; f < 2; f++) {
        if (values[f]) {
            char* at = values[f];
            for (const std::string& value : t.values[f]) {
                std::memcpy(at, value.c_str(), value.size() + 1u);
                at += value.size() + 1u;
            }
        }
        if (counts[f]) std::copy(t.counts[f].begin(), t.counts[f].end(), counts[f]);
    }
    if (row) std::copy(t.row.begin(), t.row.end(), row);
    if (column) std::copy(t.column.begin(), t.column.end(), column);
    if (count) std::copy(t.count.begin(), t.count.end(), count);
    if (sums) std::copy(t.sums, t.sums + 4, sums);
    return EM2_OK;
}

int em2_meta_data_table_cell_rows(const em2_meta_data_table* table, uint32_t* cellRow)
{
    if (!table || !cellRow) return nullArgument("em2_meta_data_table_cell_rows");
    std::copy(table->table.cellRow.begin(), table->table.cellRow.end(), cellRow);
    return EM2_OK;
}

void em2_meta_data_table_free(em2_meta_data_table* table) { delete table; }

int em2_matrix_pie_census(em2_matrix* matrix, uint32_t vertexCount, const uint64_t* cellOffsets, const uint32_t* cells, uint64_t cellCount,
                          const uint32_t* globalCellIds, uint32_t cellSetSize, const char* metaDataName, em2_pie_census** census)
{
    if (!matrix || !metaDataName || !census || (vertexCount && !cellOffsets) || (cellCount && !cells) || (cellSetSize && !globalCellIds)) {
        return nullArgument("em2_matrix_pie_census");
    }
    *census = nullptr;
    return guarded([&] {
        matrix->impl->pieCensus(vertexCount, cellOffsets, cells, cellCount, globalCellIds, cellSetSize, metaDataName, census);
    });
}

int em2_rand_index(uint64_t sumCells, uint64_t sumRows, uint64_t sumColumns, uint64_t n, double* randIndex, double* adjustedRandIndex)
{
    if (!randIndex || !adjustedRandIndex) return nullArgument("em2_rand_index");
    return guarded([&] {
        if (n == 0) throw em2::host::Error{EM2_ERROR_RUNTIME, "Assertion failed: rowCount > 0 (computeRandIndex: a table of no element)"};
        if (!em2::host::randIndexFromSums(sumCells, sumRows, sumColumns, n, *randIndex, *adjustedRandIndex)) {
            throw em2::host::Error{EM2_ERROR_UNSUPPORTED, "em2_rand_index: n (n - 1) is not below 2^53, where the reference's sums of doubles "
                                                          "stop being exact; at most 94906266 elements are supported."};
        }
    });
}

int em2_matrix_flush(em2_matrix* matrix)
{
    if (!matrix) return nullArgument("em2_matrix_flush");
    return guarded([&] { matrix->impl->flush(); });
}

int em2_tool_create_meta_data(const char* directoryName, uint32_t cellCount, uint64_t nameCapacity, uint64_t valueCapacity)
{
    if (!directoryName) return nullArgument("em2_tool_create_meta_data");
    return guarded([&] { em2::host::createMetaDataFiles(directoryName, cellCount, nameCapacity, valueCapacity); });
}

// ---- ingest (em2_ingest_host.cpp, em2_ingest.hip) ----

}  // extern "C"

namespace {

// `count` strings, each followed by its NUL, in `bytes` bytes.
std::vector<std::string> splitStrings(const char* who, const char* packed, uint64_t bytes, uint64_t count)
{
    std::vector<std::string> result;
    result.reserve(size_t(count));
    uint64_t at = 0;
    while (at < bytes && result.size() < count) {
        const void* end = std::memchr(packed + at, 0, size_t(bytes - at));
        if (!end) break;
        const uint64_t length = uint64_t(static_cast<const char*>(end) - (packed + at));
        result.emplace_back(packed + at, size_t(length));
        at += length + 1u;
    }
    if (result.size() != count || at != bytes) {
        throw em2::host::Error{EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": the packed strings are not as many as their count says"};
    }
    return result;
}

std::vector<std::pair<std::string, std::string>> splitPairs(const char* who, const char* packed, uint64_t bytes, uint64_t pairCount)
{
    const std::vector<std::string> flat = splitStrings(who, packed, bytes, 2u * pairCount);
    std::vector<std::pair<std::string, std::string>> pairs;
    for (size_t i = 0; i < flat.size(); i += 2) pairs.emplace_back(flat[i], flat[i + 1]);
    return pairs;
}

}  // namespace

extern "C" {

int em2_matrix_create(const char* directoryName, em2_matrix** matrix)
{
    if (!directoryName || !matrix) return nullArgument("em2_matrix_create");
    *matrix = nullptr;
    return guarded([&] {
        std::unique_ptr<em2::host::Matrix> m(em2::host::Matrix::create(directoryName));
        *matrix = new em2_matrix{m.get()};
        m.release();
    });
}

int em2_matrix_gene_count(em2_matrix* matrix, uint32_t* geneCount)
{
    if (!matrix || !geneCount) return nullArgument("em2_matrix_gene_count");
    return guarded([&] { *geneCount = matrix->impl->geneCount(); });
}

int em2_matrix_cell_count(em2_matrix* matrix, uint32_t* cellCount)
{
    if (!matrix || !cellCount) return nullArgument("em2_matrix_cell_count");
    return guarded([&] { *cellCount = matrix->impl->cellCount(); });
}

int em2_matrix_add_gene(em2_matrix* matrix, const char* geneName, int* added)
{
    if (!matrix || !geneName || !added) return nullArgument("em2_matrix_add_gene");
    *added = 0;
    return guarded([&] { *added = matrix->impl->addGene(geneName) ? 1 : 0; });
}

int em2_matrix_gene_name(em2_matrix* matrix, uint32_t geneId, uint64_t* bytes, char* value)
{
    if (!matrix || !bytes) return nullArgument("em2_matrix_gene_name");
    return guarded([&] { copyOut("em2_matrix_gene_name", matrix->impl->geneName(geneId), bytes, value); });
}

int em2_matrix_gene_id_from_name(em2_matrix* matrix, const char* geneName, uint32_t* geneId)
{
    if (!matrix || !geneName || !geneId) return nullArgument("em2_matrix_gene_id_from_name");
    return guarded([&] { *geneId = matrix->impl->geneIdFromName(geneName); });
}

int em2_matrix_cell_id_from_string(em2_matrix* matrix, const char* s, uint32_t* cellId)
{
    if (!matrix || !s || !cellId) return nullArgument("em2_matrix_cell_id_from_string");
    return guarded([&] { *cellId = matrix->impl->cellIdFromString(s); });
}

int em2_matrix_add_cell(em2_matrix* matrix, const char* metaData, uint64_t metaDataBytes, uint32_t metaDataPairCount,
                        const char* geneNames, uint64_t geneNamesBytes, const float* counts, uint32_t countCount, uint32_t* cellId)
{
    if (!matrix || !cellId || (!metaData && metaDataBytes) || (!geneNames && geneNamesBytes) || (!counts && countCount)) {
        return nullArgument("em2_matrix_add_cell");
    }
    return guarded([&] {
        const auto pairs = splitPairs("em2_matrix_add_cell", metaData, metaDataBytes, metaDataPairCount);
        const std::vector<std::string> names = splitStrings("em2_matrix_add_cell", geneNames, geneNamesBytes, countCount);
        std::vector<std::pair<std::string, float>> expressionCounts;
        expressionCounts.reserve(names.size());
        for (size_t i = 0; i < names.size(); i++) expressionCounts.emplace_back(names[i], counts[i]);
        *cellId = matrix->impl->addCell(pairs, expressionCounts);
    });
}

int em2_matrix_add_cells_csr(em2_matrix* matrix, const char* geneNames, uint64_t geneNamesBytes, uint32_t geneNameCount,
                             const char* cellNames, uint64_t cellNamesBytes, uint32_t cellCount, const uint64_t* indptr,
                             const uint32_t* indices, const float* values, uint64_t entryCount, const uint8_t* skip,
                             const char* cellNamePrefix, const char* cellMetaData, uint64_t cellMetaDataBytes,
                             uint32_t cellMetaDataPairCount, uint64_t chunkBytes, uint32_t* firstCellId, uint32_t* addedCellCount)
{
    if (!matrix || !indptr || !cellNamePrefix || !firstCellId || !addedCellCount || (!geneNames && geneNamesBytes) ||
        (!cellNames && cellNamesBytes) || (!cellMetaData && cellMetaDataBytes) || ((!indices || !values) && entryCount)) {
        return nullArgument("em2_matrix_add_cells_csr");
    }
    return guarded([&] {
        const char* who = "em2_matrix_add_cells_csr";
        const std::vector<std::string> genes = splitStrings(who, geneNames, geneNamesBytes, geneNameCount);
        const std::vector<std::string> cells = splitStrings(who, cellNames, cellNamesBytes, cellCount);
        const auto pairs = splitPairs(who, cellMetaData, cellMetaDataBytes, cellMetaDataPairCount);
        matrix->impl->addCellsFromCsr(genes, cells, indptr, indices, values, entryCount, skip, cellNamePrefix, pairs, chunkBytes,
                                      *firstCellId, *addedCellCount);
    });
}

int em2_matrix_add_cells_csv(em2_matrix* matrix, const char* expressionCountsFileName, const char* expressionCountsFileSeparators,
                             const char* cellMetaDataFileName, const char* cellMetaDataFileSeparators, const char* additionalCellMetaData,
                             uint64_t additionalCellMetaDataBytes, uint32_t additionalCellMetaDataPairCount, uint64_t chunkBytes,
                             int useDevice, uint32_t* firstCellId, uint32_t* addedCellCount, uint64_t* deferredFieldCount)
{
    if (!matrix || !expressionCountsFileName || !expressionCountsFileSeparators || !cellMetaDataFileName || !cellMetaDataFileSeparators ||
        !firstCellId || !addedCellCount || (!additionalCellMetaData && additionalCellMetaDataBytes)) {
        return nullArgument("em2_matrix_add_cells_csv");
    }
    return guarded([&] {
        const auto pairs = splitPairs("em2_matrix_add_cells_csv", additionalCellMetaData, additionalCellMetaDataBytes,
                                      additionalCellMetaDataPairCount);
        matrix->impl->addCellsFromCsv(expressionCountsFileName, expressionCountsFileSeparators, cellMetaDataFileName,
                                      cellMetaDataFileSeparators, pairs, chunkBytes, useDevice != 0, *firstCellId, *addedCellCount,
                                      deferredFieldCount);
    });
}

int em2_matrix_add_cell_meta_data_csv(em2_matrix* matrix, const char* cellMetaDataFileName)
{
    if (!matrix || !cellMetaDataFileName) return nullArgument("em2_matrix_add_cell_meta_data_csv");
    return guarded([&] { matrix->impl->addCellMetaDataFromFile(cellMetaDataFileName); });
}

int em2_csv_tokenize(const char* separators, const char* line, uint64_t lineBytes, int removeLeadingAndTrailingBlanks, uint64_t* tokenCount,
                     uint64_t* bytes, char* packed)
{
    if (!separators || (!line && lineBytes) || !tokenCount || !bytes) return nullArgument("em2_csv_tokenize");
    return guarded([&] {
        std::vector<std::string> tokens;
        em2::host::tokenize(separators, line, size_t(lineBytes), tokens, removeLeadingAndTrailingBlanks != 0);
        std::string all;
        for (const std::string& t : tokens) {
            all += t;
            all += '\0';
        }
        *tokenCount = tokens.size();
        copyOut("em2_csv_tokenize", all, bytes, packed);
    });
}

}  // extern "C"
